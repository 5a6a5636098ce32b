"""GPU: solve sessions on libnbp (schedules compiled by the native host) against sessions on the oracle backend (the Python
mirror's schedules) with the same seeds -- the scenarios of tests/session_cases.py, the ones tests/test_session.py runs on
the oracle alone.  After every solve every belief is identical bit for bit between the two sessions -- SE(2) included, where
both sides keep theta resident -- the two sessions moved the same beliefs, and the residency audit finds in every variable
slot of both backends exactly the host's belief.  On Euclid and Circular graphs the libnbp session also equals
solveTree(backend = libnbp, oldtree = ...) on a third copy, getPPESuggested included."""
import pytest

import session_cases as sc

pytestmark = pytest.mark.gpu


def test_chain24_grown_by_four_poses(oracle_backend, hip_backend):
    sc.chain24_grown_by_four([oracle_backend, hip_backend], hip_backend)


def test_marginalization_scenario(oracle_backend, hip_backend):
    sc.marginalization_scenario([oracle_backend, hip_backend], hip_backend)


def test_traffic_counts(oracle_backend, hip_backend):
    sc.traffic_counts([oracle_backend, hip_backend], hip_backend)


@pytest.mark.parametrize("how", ["setValKDE", "in_place"])
def test_host_edits_win(oracle_backend, hip_backend, how):
    sc.host_edits_win([oracle_backend, hip_backend], hip_backend, how)


def test_in_place_edit_without_invalidate_is_not_seen(oracle_backend, hip_backend):
    sc.in_place_edit_without_invalidate_is_not_seen([oracle_backend, hip_backend])


def test_context_grows(oracle_backend, hip_backend):
    sc.context_grows([oracle_backend, hip_backend], hip_backend)


def test_deleted_variable_renumbers_the_slots(oracle_backend, hip_backend):
    sc.deleted_variable_renumbers_the_slots([oracle_backend, hip_backend], hip_backend)


def test_graph_initialisation_runs_in_the_session_context(oracle_backend, hip_backend):
    sc.graph_initialisation_runs_in_the_session_context([oracle_backend, hip_backend], hip_backend)


def test_initialised_but_not_updated_beliefs_reach_the_host(oracle_backend, hip_backend):
    sc.initialised_but_not_updated([oracle_backend, hip_backend], hip_backend)


def test_failed_program_clears_the_table_and_the_context_lives_on(oracle_backend, hip_backend):
    """the failure is a Python exception raised in front of the launch: nothing faults on the device"""
    sc.failed_program_clears_the_table_and_the_context_lives_on([oracle_backend, hip_backend], hip_backend)


def test_se2_chain_with_fixed_lag(oracle_backend, hip_backend):
    sc.se2_chain_with_fixed_lag([oracle_backend, hip_backend])


def test_circular_chain_across_the_cut(oracle_backend, hip_backend):
    sc.circular_chain([oracle_backend, hip_backend], hip_backend)


@pytest.mark.parametrize("N", [65, 37])
def test_count_edges(oracle_backend, hip_backend, N):
    """particle counts that are no multiple of the wave, through the batched reads and writes and run_ppe over resident slots"""
    sc.count_edges([oracle_backend, hip_backend], hip_backend, N)


def test_passthrough_density_se2(oracle_backend, hip_backend):
    """SE(2): the session is its own definition (a resident belief keeps theta), so there is no comparison bit for bit with
    solveTree: the two sessions are identical, the audit holds, and every estimate is that of the host belief"""
    sc.passthrough_density([oracle_backend, hip_backend], None, "se2")


def test_passthrough_density_euclid2(oracle_backend, hip_backend):
    sc.passthrough_density([oracle_backend, hip_backend], hip_backend, "euclid2")


def test_mixed_graph_grown_twice(oracle_backend, hip_backend):
    sc.mixed_graph_grown_twice([oracle_backend, hip_backend], hip_backend)
