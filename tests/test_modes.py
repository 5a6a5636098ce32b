"""Modes of a belief on the host: the numpy restatement of the definition (incrementalinference.jl_amd/modes.py) against the
table of tests/modes_cases.py -- the number of modes every cloud must have --, the mirror without a backend, the refusals of the
options and the ranking's tie rule."""
import numpy as np
import pytest

import modes_cases as mc
import ppe_cases as pc
from parity_utils import abi, iif

modes = iif.modes


@pytest.mark.parametrize("N", mc.SIZES)
def test_every_cloud_has_the_modes_the_table_requires(N):
    rng = np.random.default_rng(300 + N)
    for m in mc.MANIFOLDS:
        for kind in mc.TABLE_CLOUDS + (("doors4",) if m == abi.CIRCULAR else ()):
            X, bw, scale, heavy = mc.make(kind, m, N, rng)
            bm = modes.modes_numpy(m, pc.to_points(m, X), bw, scale, mc.TOL, mc.MAX_ITER, mc.MERGE)
            Xc = modes.ppe_coords(m, pc.to_points(m, X))  # (SE(2): the heading as it comes back from the rotation matrix)
            mc.check_table(kind, m, Xc, bm, heavy, f"manifold {m} N={N}")
            assert bm.modes.shape == (bm.n_modes, abi.MANIFOLD_DIM[m]) and bm.density.shape == (bm.n_modes,)
            assert np.all(np.diff(bm.counts) <= 0) and abs(bm.shares.sum() - 1) < 1e-15 * N


def test_one_point_is_its_own_mode():
    rng = np.random.default_rng(1)
    for m in mc.MANIFOLDS:
        X = pc.cloud("gaussian", m, 1, rng)
        bm = modes.modes_numpy(m, pc.to_points(m, X), pc.hand_bandwidth(m))
        mc.check_table("identical", m, modes.ppe_coords(m, pc.to_points(m, X)), bm, what=f"manifold {m} one point")
        D = abi.MANIFOLD_DIM[m]
        assert abs(bm.density[0] * np.prod(2.0 * pc.hand_bandwidth(m) * np.sqrt(2 * np.pi)) - 1) < 1e-15 * 4 * D


def test_doors_are_found_where_they_stand_with_their_shares():
    rng = np.random.default_rng(2)
    X, bw, scale, _ = mc.make("doors4", abi.CIRCULAR, 1000, rng)
    bm = modes.modes_numpy(abi.CIRCULAR, X, bw, scale)
    assert bm.n_modes == 4
    # the shares are binomial draws of 1000: three standard deviations of the largest are 0.046; the lightest door holds ~100
    # points of sigma 0.1: four standard errors of their mean are 0.04
    assert np.abs(pc.wrap(bm.modes[:, 0] - np.asarray(mc.DOORS))).max() < 0.04, bm.modes
    assert np.abs(bm.shares - np.asarray(mc.DOOR_SHARES)).max() < 0.05, bm.shares


def test_bad_bandwidth_has_no_modes():
    rng = np.random.default_rng(3)
    for m in mc.MANIFOLDS:
        X = pc.cloud("gaussian", m, 50, rng)
        for bad in (0.0, np.nan, np.inf, -1.0):
            bw = pc.hand_bandwidth(m).copy()
            bw[-1] = bad
            bm = modes.modes_numpy(m, pc.to_points(m, X), bw)
            assert bm.n_modes == 0 and len(bm.modes) == 0 and np.all(bm.labels == -1) and len(bm.labels) == 50 and np.all(bm.iters == 0)


def test_max_iter_is_reported():
    rng = np.random.default_rng(4)
    X = pc.cloud("two_cluster", abi.EUCLID2, 100, rng)
    bm = modes.modes_numpy(abi.EUCLID2, X, pc.hand_bandwidth(abi.EUCLID2), 1.0, mc.TOL, 3, mc.MERGE)
    assert bm.n_unconverged > 0 and bm.iters.max() == 3 and np.all(bm.iters[bm.iters < 3] >= 1)


def test_equal_counts_rank_by_the_lower_leader():
    """50 / 50: the cluster that holds point 0 comes first whichever side it lies on"""
    rng = np.random.default_rng(5)
    for first in (-1.0, 1.0):
        side = np.where(np.arange(100) % 2 == 0, first, -first)
        X = side[:, None] + rng.normal(0, 0.2, (100, 2))
        bm = modes.modes_numpy(abi.EUCLID2, X, pc.hand_bandwidth(abi.EUCLID2), 1.0)
        assert bm.n_modes == 2 and bm.counts.tolist() == [50, 50] and bm.leader.tolist() == [0, 1]
        assert np.array_equal(bm.labels, np.arange(100) % 2)
        assert np.sign(bm.modes[0, 0]) == first and np.sign(bm.modes[1, 0]) == -first
    # ... and a heavier cluster comes first even when it holds the higher indices
    side = np.where(np.arange(100) < 30, -1.0, 1.0)
    X = side[:, None] + rng.normal(0, 0.2, (100, 2))
    bm = modes.modes_numpy(abi.EUCLID2, X, pc.hand_bandwidth(abi.EUCLID2), 1.0)
    assert bm.counts.tolist() == [70, 30] and bm.leader.tolist() == [30, 0] and np.array_equal(bm.labels, (np.arange(100) < 30).astype(int))


def test_options_are_validated():
    X, bw = np.zeros((4, 1)), [0.1]
    for kw in (dict(bw_scale=0.0), dict(bw_scale=np.inf), dict(bw_scale=np.nan), dict(tol=0.0), dict(tol=-1.0), dict(max_iter=0),
               dict(merge=0.0), dict(merge=np.nan), dict(tol=1e-4, merge=1e-2), dict(merge=9.99e-4)):
        with pytest.raises(ValueError):
            modes.modes_numpy(abi.EUCLID1, X, bw, **kw)
    modes.modes_numpy(abi.EUCLID1, X, bw, tol=1e-5, merge=1e-2)  # merge = 1000 tol is admitted


def test_the_mirror_without_a_backend():
    fg = iif.initfg(iif.SolverParams(N=80))
    iif.addVariable(fg, "x0", iif.ContinuousScalar)
    iif.addVariable(fg, "x1", iif.Circular)
    rng = np.random.default_rng(6)
    X0 = np.where(np.arange(80)[:, None] < 60, -1.0, 1.0) + rng.normal(0, 0.1, (80, 1))
    X1, bw1, _, _ = mc.make("doors4", abi.CIRCULAR, 80, rng)
    iif.setValKDE(fg, "x0", X0, [0.15])
    iif.setValKDE(fg, "x1", X1, bw1)
    bm = iif.getBeliefModes(fg, "x0", bwScale=1.0)
    assert isinstance(bm, iif.BeliefModes) and bm.n_modes == 2 and bm.counts.tolist() == [60, 20]
    assert np.array_equal(bm.shares, [0.75, 0.25]) and abs(bm.modes[0, 0] + 1) < 0.05 and abs(bm.modes[1, 0] - 1) < 0.08
    ref = iif.modes_numpy(abi.EUCLID1, X0, [0.15], 1.0)
    assert ref.modes.tobytes() == bm.modes.tobytes() and np.array_equal(ref.labels, bm.labels)
    both = iif.getBeliefModesAll(fg)
    assert list(both) == ["x0", "x1"] and both["x1"].n_modes == iif.modes_numpy(abi.CIRCULAR, X1, bw1).n_modes
    assert both["x0"].modes.tobytes() == iif.getBeliefModes(fg, "x0").modes.tobytes()
    b = iif.getBelief(fg, "x0")
    assert b.modes(bwScale=1.0).modes.tobytes() == bm.modes.tobytes()
    with pytest.raises(ValueError):
        iif.getBeliefModes(fg, "x0", merge=1e-4)
    with pytest.raises(ValueError):
        b.modes(maxIter=0)
