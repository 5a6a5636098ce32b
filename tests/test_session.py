"""CPU: solve sessions (iif.SolveSession) on the oracle backend -- a session solve is solveTree(oldtree = the last tree) with
the beliefs resident between solves.  Every scenario (tests/session_cases.py, shared with tests/test_gpu_session.py) runs
through a session on one graph and through solveTree on a twin with the same seeds; on Euclid and Circular graphs the two are
identical bit for bit.  The traffic counts are known answers: what is new or edited goes up, what a program updated comes
down.  Behind every solve the residency audit reads the backend's slots: each holds exactly the host's belief."""
import numpy as np
import pytest

import incremental_cases as cases
import session_cases as sc
from oracle.oracle_backend import OracleBackend
from parity_utils import iif


def oracle(N, n_slots, side_ints=0):
    return OracleBackend(N, n_slots, side_ints, threads=8)


# ---- 1: the chain grown by four ------------------------------------------------------------------------------------------------
def test_chain24_grown_by_four_equals_solvetree():
    sc.chain24_grown_by_four([oracle], oracle)


# ---- 2: the marginalization scenario of the reference ---------------------------------------------------------------------------
def test_marginalization_scenario_equals_solvetree():
    sc.marginalization_scenario([oracle], oracle)


# ---- 3: traffic ----------------------------------------------------------------------------------------------------------------------
def test_traffic_counts():
    sc.traffic_counts([oracle], oracle)


def test_frozen_variables_do_not_travel(monkeypatch):
    fg = cases.chain24(n=30)
    writes, reads = [], []
    real_write, real_read = OracleBackend.belief_write, OracleBackend.belief_read
    monkeypatch.setattr(OracleBackend, "belief_write", lambda self, slot, *a, **k: (writes.append(slot), real_write(self, slot, *a, **k))[1])
    monkeypatch.setattr(OracleBackend, "belief_read", lambda self, slot, *a, **k: (reads.append(slot), real_read(self, slot, *a, **k))[1])
    with iif.SolveSession(fg, backend=oracle, reserve=500) as ses:
        ses.solve(seed=1, eliminationOrder=fg.ls())
        assert sorted(writes) == list(range(30)) == sorted(reads)
        sc.audit_residency(ses, fg.ls())
        iif.defaultFixedLagOnTree(fg, 6)
        cases.grow_chain(fg, 2)
        before = {v: (fg.getVal(v), fg.getVariable(v).bw) for v in fg.ls()}
        table = dict(ses._table)
        del writes[:], reads[:]
        tree = ses.solve(seed=2, eliminationOrder=fg.ls())
        frozen = [i for i, v in enumerate(fg.ls()) if fg.getVariable(v).ismargin]
        assert frozen == list(range(26))  # all but the last six of the add history
        assert sorted(writes) == [30, 31]
        assert not set(reads) & set(frozen) and set(reads) == set(range(26, 32))
        assert ses.stats["last"] == {"uploads": 2, "readbacks": 6, "resyncs": 0}
        for i in frozen:  # not even the array objects changed
            v = fg.ls()[i]
            assert fg.getVal(v) is before[v][0] and fg.getVariable(v).bw is before[v][1]
            assert ses._table[i] is table[i]
        assert iif.calcCliquesRecycled(tree)[1] >= 20
        sc.audit_residency(ses, fg.ls(), table)  # (the audit's own reads come last: the lists above are the solve's)


# ---- 4: host edits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["setValKDE", "in_place"])
def test_host_edits_win(how):
    sc.host_edits_win([oracle], oracle, how)


def test_in_place_edit_without_invalidate_is_not_seen():
    sc.in_place_edit_without_invalidate_is_not_seen([oracle])


# ---- 5: growth ------------------------------------------------------------------------------------------------------------------------
def test_context_grows():
    sc.context_grows([oracle], oracle)


# ---- 6: renumbering ----------------------------------------------------------------------------------------------------------------
def test_deleted_variable_renumbers_the_slots():
    sc.deleted_variable_renumbers_the_slots([oracle], oracle)


def test_graph_initialisation_runs_in_the_session_context():
    sc.graph_initialisation_runs_in_the_session_context([oracle], oracle)


def test_initialised_but_not_updated_beliefs_reach_the_host():
    sc.initialised_but_not_updated([oracle], oracle)


# ---- 7: errors and closing -------------------------------------------------------------------------------------------------------------
def test_joint_messages_first_solve_runs_second_raises():
    fg = cases.marginalization_graph()
    for v in [v for v in fg.ls() if v not in ("x0", "x1", "x2")]:
        iif.deleteVariable(fg, v)
    fg.solverParams.useMsgLikelihoods = True
    ses = iif.SolveSession(fg, backend=oracle)
    ses.solve(seed=31)
    sc.audit_residency(ses, fg.ls())
    cases.assert_ppe_band(fg, "joint")
    with pytest.raises(ValueError, match="useMsgLikelihoods"):
        ses.solve(seed=32)
    sc.audit_residency(ses, fg.ls())  # refused before anything moved
    ses.close()
    ses.close()
    with pytest.raises(RuntimeError, match="closed"):
        ses.solve(seed=33)


def test_failed_program_clears_the_table_and_the_context_lives_on():
    sc.failed_program_clears_the_table_and_the_context_lives_on([oracle], oracle)
    with pytest.raises(TypeError):
        iif.SolveSession(cases.chain24(n=8), backend=oracle(100, 4))


# ---- 8: SE(2) ----------------------------------------------------------------------------------------------------------------------
def test_se2_chain_with_fixed_lag():
    sc.se2_chain_with_fixed_lag([oracle])


# ---- Circular: the contract says bit-identical --------------------------------------------------------------------------------------
def test_circular_chain_equals_solvetree():
    sc.circular_chain([oracle], oracle)


# ---- particle counts, density slots, mixed factors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 37])
def test_count_edges(N):
    sc.count_edges([oracle], oracle, N)


def test_passthrough_density_se2():
    """SE(2): the session is its own definition (a resident belief keeps theta), so there is no comparison bit for bit with
    solveTree; the audit and the estimates hold it"""
    sc.passthrough_density([oracle], None, "se2")


def test_passthrough_density_euclid2_equals_solvetree():
    sc.passthrough_density([oracle], oracle, "euclid2")


def test_mixed_graph_grown_twice_equals_solvetree():
    sc.mixed_graph_grown_twice([oracle], oracle)
