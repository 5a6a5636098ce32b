"""-m gpu: every kernel a proposal launch can run, at the edges of its geometry, held to the oracle.

What a proposal launch runs is decided on the host (proposal_plan in csrc/nbp_api.hip): one of the five workgroup instances, of
the three one-wave-per-proposal kernels, or the two-waves-per-proposal kernel.  The cases (tests/proposal_geometry_cases.py,
checked on the CPU by tests/test_proposal_geometry_cases.py) run each at the particle counts on either side of every chunk of 64,
in batches that fill a workgroup of waves exactly, partly and by one too many, with every descriptor kind of the class: relatives
solving either variable, short operands and targets, mixtures, priors, message priors, and the pass-through branch -- written out
once per geometry -- with keep_count 0, 1 and 2.  Every case

  * creates its context under its option set (the switches are read at context creation) and asserts that its one launch ran the
    geometry it was chosen for (nbp_diag: proposal_launches_workgroup / _wave / _split), and that the planner names its kernel
    under the same options -- a case whose launch ran another kernel fails instead of passing on it;
  * runs the same batch on the oracle: the raw rows of every output slot, the bandwidths, infoPerCoord, the count, the hypothesis
    indices and the side memory no descriptor names, the solves and the residual evaluations -- equal, no tolerance anywhere."""
import numpy as np
import pytest

import proposal_geometry_cases as pgc
from launch_plan_cases import options
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu


def _hip_under(env):
    def make(N, n_slots, side_ints=0):
        with options(env):
            return iif.HipBackend(N, n_slots, side_ints=side_ints)
    return make


def _where(a, b, N):
    """which particles differ: indices, chunks of 64, lanes"""
    bad = np.flatnonzero((a != b).any(axis=1))
    if not bad.size:
        return "no particle differs"
    return (f"{bad.size} of {N} particles differ (first {bad[:8].tolist()}), chunks {sorted(set((bad // 64).tolist()))}, lanes {int((bad % 64).min())}..{int((bad % 64).max())}, "
            f"max |difference| {np.nanmax(np.abs(a - b)):.3e}")


@pytest.mark.parametrize("case", pgc.cases(), ids=lambda c: c["id"])
def test_the_launch_of_every_geometry_equals_the_oracle(case):
    N, env = case["N"], pgc.OPTION_SETS[case["options"]]
    _, descs, names = pgc.case_batch(case)
    with options(env):
        plan = abi.plan_proposals([(N, len(descs), case["man"], 1)])[0]
    assert (plan.kernel.decode(), plan.geometry) == (case["kernel"], pgc.GEOMETRY[case["want"]])
    got = pgc.run_case(_hip_under(env), case)
    dg = got["diag"]
    ran = (dg["proposal_launches_workgroup"], dg["proposal_launches_wave"], dg["proposal_launches_split"])
    assert ran == pgc.LAUNCHES[case["geometry"]], f"the launch did not run the geometry this case was chosen for ({case['kernel']}): {ran}"
    want = pgc.oracle_of(case)
    for j, (name, d) in enumerate(zip(names, descs)):
        what = f"descriptor {j} {name} (kind {d.factor_kind}, sfidx {d.sfidx}, cycles {d.inflate_cycles}, keep_count {d.keep_count})"
        assert np.array_equal(got["rows"][j], want["rows"][j]), f"{what}: {_where(got['rows'][j], want['rows'][j], N)}"
        assert np.array_equal(got["bw"][j], want["bw"][j]), f"{what}: bandwidths {got['bw'][j]} / {want['bw'][j]}"
        assert np.array_equal(got["ipc"][j], want["ipc"][j]), f"{what}: infoPerCoord {got['ipc'][j]} / {want['ipc'][j]}"
        assert got["count"][j] == want["count"][j], f"{what}: count {got['count'][j]} / {want['count'][j]}"
        if d.mhidx_out >= 0:
            assert np.array_equal(got["side"][d.mhidx_out:d.mhidx_out + N], want["side"][d.mhidx_out:d.mhidx_out + N]), f"{what}: hypothesis indices"
    named = np.zeros(3 * N, dtype=bool)
    for d in descs:
        if d.mhidx_out >= 0:
            named[d.mhidx_out:d.mhidx_out + N] = True
    assert (got["side"][~named] == pgc.SIDE_SENTINEL).all(), "side memory no descriptor names was written"
    assert np.array_equal(got["side"], want["side"])
    assert (dg["solves"], dg["residual_evals"]) == (want["diag"]["solves"], want["diag"]["residual_evals"]), (dg, want["diag"])
