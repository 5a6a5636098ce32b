"""Launches of "simple" Euclid(2) proposals (LinearRelative between two variables, no multihypo, no nullhypo; priors, message
priors and pass-through densities ride along) that are too small for one wave per proposal and too large for the workgroup
kernel run TWO waves per proposal (nbp_proposal_split_kernel_lin2): wave w of the workgroup owns the chunks w, w + 2 of 64
particles, the spread statistics add the chunk partials in chunk order through LDS.  The particles must not depend on the
geometry: compared with the workgroup kernel BIT FOR BIT, with as many searches and residual evaluations.

Selection (launch_proposals in nbp_api.hip), read from the environment when the context is created:
  NBP_PROPOSAL_WAVE_MIN=n   from n proposals per launch on: one wave per proposal.  It keeps its precedence: with
                            NBP_PROPOSAL_WAVE_MIN=1 every simple batch runs the one-wave kernel, whatever
                            NBP_PROPOSAL_SPLIT_MIN says.
  NBP_PROPOSAL_SPLIT_MIN=m  m <= proposals < wave minimum: the split kernel; below m: the workgroup kernel.
Which kernel a launch ran is read from nbp_diag: proposal_launches_workgroup / _wave / _split."""
import os

import numpy as np
import pytest

from parity_utils import abi, iif, rand_points, relative_factor_desc

pytestmark = pytest.mark.gpu

MAN, DIM = abi.EUCLID2, 2
ENV = ("NBP_PROPOSAL_WAVE_MIN", "NBP_PROPOSAL_SPLIT_MIN")


def _backend(N, env):
    """a context created under exactly the switches of `env` (both variables unset otherwise, and afterwards)"""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(env)
    try:
        return iif.HipBackend(N, 24, N)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _batch(N, rng, be):
    # slots 0..5: beliefs; slot 3 holds fewer points than N (a target copy resized to N / an operand read through
    # _getindex_anyn); slot 5: a density for the pass-through proposal
    for j in range(6):
        pts = rand_points(rng, MAN, N if j != 3 else max(2, N - 37), 1.5 * j, 0.4)
        be.belief_write(j, MAN, pts, np.full(DIM, 0.3))
    mean, sig = [1.0, -0.5], [0.1, 0.2]
    descs = [
        relative_factor_desc(abi.F_LINREL, MAN, 2, 1, [0, 1], 8, 11, mean, sig),              # solve the second variable
        relative_factor_desc(abi.F_LINREL, MAN, 2, 0, [2, 4], 9, 12, mean, sig),              # solve the first
        relative_factor_desc(abi.F_LINREL, MAN, 2, 1, [3, 2], 10, 13, mean, sig),             # operand with fewer points
        relative_factor_desc(abi.F_LINREL, MAN, 2, 0, [3, 1], 11, 14, mean, sig, cycles=2),   # target with fewer points
        relative_factor_desc(abi.F_PRIOR, MAN, 1, 0, [0], 12, 15, mean, sig),
        relative_factor_desc(abi.F_MSGPRIOR, MAN, 1, 0, [0, 1], 13, 16, [0], [0]),
        relative_factor_desc(abi.F_MSGPRIOR, MAN, 1, 0, [2, 3], 14, 17, [0], [0]),            # message with fewer points
        relative_factor_desc(abi.F_LINREL, MAN, 2, 1, [4, 0], 15, 18, mean, sig, mhidx_out=0),
        relative_factor_desc(abi.F_PASSTHROUGH, MAN, 1, 0, [1, 5], 16, 19, [0], [0]),
    ]
    return descs


def _run(N, env, pick=None):
    be = _backend(N, env)
    descs = _batch(N, np.random.default_rng(5), be)
    if pick is not None:
        descs = [descs[i] for i in pick]
    be.diag(reset=True)
    be.run_proposals(descs)
    dg = be.diag()
    res = ([be.slot_read(d.out_slot, MAN) for d in descs], np.array(be.side_read(0, N)), dg)
    be.close()
    return res


def _assert_same(a, b, what):
    (sa, mha, dga), (sb, mhb, dgb) = a, b
    assert np.array_equal(mha, mhb), what
    assert dga["solves"] == dgb["solves"] and dga["residual_evals"] == dgb["residual_evals"], (what, dga, dgb)
    assert len(sa) == len(sb)
    for (pa, ba), (pb, bb) in zip(sa, sb):
        assert pa.shape == pb.shape
        assert np.array_equal(pb, pa) and np.array_equal(bb, ba), f"{what}: max |difference| {np.abs(pa - pb).max():.3e}"


SPLIT = {"NBP_PROPOSAL_SPLIT_MIN": "1"}


# 64: the second wave owns no chunk; 65: a chunk of one particle; 129: three chunks; 150, 200: a partial last chunk; 256: all full
@pytest.mark.parametrize("N", [64, 65, 129, 150, 200, 256])
def test_split_geometry_equals_workgroup_geometry(N):
    wg, sp = _run(N, {}), _run(N, SPLIT)
    assert sp[2]["proposal_launches_split"] == 1 and sp[2]["proposal_launches_workgroup"] == 0, sp[2]
    assert wg[2]["proposal_launches_workgroup"] == 1 and wg[2]["proposal_launches_split"] == 0, wg[2]
    assert (sp[1] == 1).all()
    _assert_same(wg, sp, f"N {N}")


@pytest.mark.parametrize("pick", [[7], None], ids=["batch1", "batch9"])
def test_batch_sizes(pick):
    # the grid is the batch: one workgroup per proposal, none partial
    wg, sp = _run(200, {}, pick), _run(200, SPLIT, pick)
    assert sp[2]["proposal_launches_split"] == 1
    _assert_same(wg, sp, f"batch {pick}")


def _launches(env, nullhypo=False):
    be = _backend(200, env)
    descs = _batch(200, np.random.default_rng(5), be)
    if nullhypo:
        d = relative_factor_desc(abi.F_LINREL, MAN, 2, 1, [0, 1], 8, 11, [1.0, -0.5], [0.1, 0.2], nullhypo=0.1)
        descs = [d]
    be.diag(reset=True)
    be.run_proposals(descs)
    dg = be.diag()
    be.close()
    return dg["proposal_launches_workgroup"], dg["proposal_launches_wave"], dg["proposal_launches_split"]


def test_selection():
    assert _launches({}) == (1, 0, 0)                                                     # nine proposals: the workgroup kernel
    assert _launches({"NBP_PROPOSAL_WAVE_MIN": "1"}) == (0, 1, 0)
    assert _launches({"NBP_PROPOSAL_WAVE_MIN": "1", "NBP_PROPOSAL_SPLIT_MIN": "1"}) == (0, 1, 0)   # the wave minimum goes first
    assert _launches({"NBP_PROPOSAL_WAVE_MIN": "1", "NBP_PROPOSAL_SPLIT_MIN": "100000"}) == (0, 1, 0)
    assert _launches(SPLIT) == (0, 0, 1)
    # a batch that is not simple never runs it
    for env in ({}, SPLIT, {"NBP_PROPOSAL_WAVE_MIN": "1", "NBP_PROPOSAL_SPLIT_MIN": "1"}):
        assert _launches(env, nullhypo=True) == (1, 0, 0), env


def _solve(env):
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(env)
    try:
        fg = iif.generateChainEuclid(60, vardims=2, priorEvery=15, N=200)
        iif.solveTree(fg, eliminationOrder=iif.nestedDissectionOrder(fg), backend=iif.HipBackend, seed=3)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return [(fg.getVal(f"x{i}"), np.asarray(fg.getVariable(f"x{i}").bw)) for i in range(60)]


def test_whole_solve_split_equals_default_selection():
    # up and down solve of a 60-variable chain: every simple batch on the split kernel against the default selection
    a, b = _solve({}), _solve(SPLIT)
    for i, ((pa, ba), (pb, bb)) in enumerate(zip(a, b)):
        assert np.isfinite(pa).all()
        assert np.array_equal(pa, pb) and np.array_equal(ba, bb), i
