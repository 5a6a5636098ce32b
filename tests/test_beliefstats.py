"""CPU: the numpy restatements of the belief statistics (incrementalinference.jl_amd/beliefstats.py) against closed forms, the
mirror on the checker backend (which has no such entry point: numpy), and the wrap condition of tests/stats_cases.py for the seeds
tests/test_gpu_beliefstats.py uses."""
import math

import numpy as np
import pytest

import ppe_cases as pc
import stats_cases as sc
from parity_utils import abi, iif

bs = iif.beliefstats


@pytest.mark.parametrize("D", [1, 2, 3])
def test_meancov_numpy_matches_numpy_cov(D):
    man = (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3)[D - 1]
    rng = np.random.default_rng(D)
    for c in (2, 65, 200):
        X = rng.normal(0.3, 0.5, (c, D)) @ rng.normal(size=(D, D))
        mean, cov = bs.meancov_numpy(man, X)
        want = np.cov(X.T).reshape(D, D)
        assert np.abs(mean - X.mean(axis=0)).max() <= 1e-12
        assert np.abs(cov - want).max() <= 1e-12 * np.abs(want).max(), (c, cov, want)
        assert np.array_equal(cov, cov.T)
    mean, cov = bs.meancov_numpy(man, X[:1])
    assert np.array_equal(mean, X[0]) and np.isnan(cov).all() and cov.shape == (D, D)


def test_meancov_numpy_wraps_circular_clusters():
    rng = np.random.default_rng(5)
    U = rng.normal(np.pi, 0.3, (200, 1))  # unwrapped: a cluster across +-pi
    mean, cov = bs.meancov_numpy(abi.CIRCULAR, pc.wrap(U))
    assert abs(cov[0, 0] - np.var(U[:, 0], ddof=1)) <= 1e-12, (cov, np.var(U[:, 0], ddof=1))
    assert abs(pc.wrap(mean[0] - U.mean())) <= 1e-12
    # the heading of SE(2): the same cluster beside two Euclidean coordinates, through the rotation-matrix host form
    X = np.concatenate([rng.normal(0.0, 1.0, (200, 2)), pc.wrap(U)], axis=1)
    mean, cov = bs.meancov_numpy(abi.SE2, pc.to_points(abi.SE2, X))
    assert abs(cov[2, 2] - np.var(U[:, 0], ddof=1)) <= 1e-12
    assert np.abs(cov[:2, :2] - np.cov(X[:, :2].T)).max() <= 1e-12


def _log_normal_pdf(d, h):
    return -0.5 * (d / h) ** 2 - math.log(math.sqrt(2 * math.pi) * h)


@pytest.mark.parametrize("man", sc.MANIFOLDS)
def test_kld_numpy_single_point_closed_form(man):
    """a = {x} with h_a, b = {y} with h_b: kld = sum_d log N(0; 0, h_a) - log N(x - y; 0, h_b), x - y across pi where it wraps"""
    D = abi.MANIFOLD_DIM[man]
    x, y = np.array([0.7, -1.0, 0.2])[:D], np.array([0.2, -0.6, 0.5])[:D]
    ha, hb = np.array([0.3, 0.4, 0.2])[:D], np.array([0.5, 0.25, 0.35])[:D]
    for k in pc.circular_coords(man):
        x[k], y[k] = 3.0, -3.0
    d = x - y
    for k in pc.circular_coords(man):
        d[k] = 6.0 - 2 * math.pi  # across pi
    want = sum(_log_normal_pdf(0.0, ha[k]) for k in range(D)) - sum(_log_normal_pdf(d[k], hb[k]) for k in range(D))
    got = bs.kld_numpy(man, x[None, :], ha, y[None, :], hb)
    assert abs(got - want) <= 1e-14, (got, want)


def test_kld_numpy_properties():
    rng = np.random.default_rng(9)
    for man in sc.MANIFOLDS:
        D = abi.MANIFOLD_DIM[man]
        h = pc.hand_bandwidth(man)
        A = pc.cloud("gaussian", man, 120, rng)
        assert bs.kld_numpy(man, A, h, A, h) == 0.0
        assert bs.kld_numpy(man, A, h, A.copy(), h.copy()) == 0.0
        # (a resubstitution estimate, not the divergence of two densities: it has no clamp and is not >= 0 in general -- b a
        # subset of a, say, comes out a little below zero.  On clouds that differ it is positive.)
        for B, hb in ((pc.cloud("gaussian", man, 80, rng) + 0.5, h), (pc.cloud("two_cluster", man, 120, rng), 2 * h)):
            for k in pc.circular_coords(man):
                B[:, k] = pc.wrap(B[:, k])
            assert bs.kld_numpy(man, A, h, B, hb) >= -1e-12, (man, bs.kld_numpy(man, A, h, B, hb))
        assert math.isnan(bs.kld_numpy(man, A, h * 0, A, h)) and math.isnan(bs.kld_numpy(man, A, h, A, np.full(D, np.inf)))
    # b 1000 bandwidths away: the density is 0.0, its logarithm finite
    for man in (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3):
        D = abi.MANIFOLD_DIM[man]
        h = np.full(D, 0.1)
        A = rng.normal(0.0, 0.1, (50, D))
        B = A[:30] + 1000 * h
        assert np.all(iif.density_numpy(man, B, h, A) == 0.0)
        v = bs.kld_numpy(man, A, h, B, h)
        assert math.isfinite(v) and 0.4e6 * D < v < 0.6e6 * D, v


def _readme_chain(N=100):
    fg = iif.initfg(iif.SolverParams(N=N))
    for i in range(6):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
    iif.addFactor(fg, ["x0"], iif.Prior(iif.Normal(0.0, 1.0)))
    for i in range(5):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    return fg


def test_mirror_on_the_checker_backend(oracle_backend):
    assert not hasattr(oracle_backend(8, 2), "run_meancov")  # the checker has no such entry point: everything below is numpy
    fg = _readme_chain()
    with iif.SolveSession(fg, backend=oracle_backend) as ses:
        ses.solve(seed=81)
        before = {k: ses.stats[k] for k in ("uploads", "readbacks")}
        got = ses.calcMeanCovar()
        assert {k: ses.stats[k] for k in before} == before
        assert list(got) == fg.ls()
        for v in fg.ls():
            mu, Sig = iif.calcMeanCovar(fg, v, backend=oracle_backend)
            mu_n, Sig_n = bs.meancov_numpy(abi.EUCLID1, fg.getVal(v))
            assert np.array_equal(mu, mu_n) and np.array_equal(Sig, Sig_n)
            assert np.array_equal(got[v][0], mu) and np.array_equal(got[v][1], Sig)
    mu, Sig = iif.calcMeanCovar(fg, "x5")
    print("x5:", mu, Sig)
    assert mu.shape == (1,) and Sig.shape == (1, 1)
    assert 0.01 < Sig[0, 0] < 1.0 and abs(mu[0] - 5) < 0.5
    allv = iif.calcMeanCovarAll(fg, backend=oracle_backend)
    assert list(allv) == fg.ls() and np.array_equal(allv["x5"][1], Sig)
    b0, b1 = iif.getBelief(fg, "x0"), iif.getBelief(fg, "x1")
    k = iif.kld(b0, b1, iif.ContinuousScalar, backend=oracle_backend)
    assert k == bs.kld_numpy(abi.EUCLID1, b0.pts, b0.bw, b1.pts, b1.bw) and k > 0
    assert iif.kld(b0, (b1.pts, b1.bw), abi.EUCLID1) == k
    assert iif.kld(b0, b0, iif.ContinuousScalar) == 0.0
    assert iif.entropy(b0, iif.ContinuousScalar, backend=oracle_backend) == -bs.kld_terms_numpy(abi.EUCLID1, b0.pts, b0.bw, b0.pts, b0.bw)[0]
    with pytest.raises(ValueError):
        iif.kld(b0.pts, b1, iif.ContinuousScalar)  # points alone carry no bandwidth
    with pytest.raises(ValueError):
        iif.kld(b0, (b1.pts, None), iif.ContinuousScalar)


def test_seeds_of_the_device_tests_meet_the_wrap_condition():
    """what tests/test_gpu_beliefstats.py asserts before it compares, here with meancov_numpy's own mean on the clouds as drawn"""
    least = np.inf
    sets = [(sc.full_items(N), 100 + N) for N in sc.FULL_COUNTS] + [(sc.below_items(), 7), (sc.batch_items(300, 200, 21), 22)]
    for items, seed in sets:
        for (m, kind, c), X in zip(items, sc.clouds(items, seed)):
            if not pc.circular_coords(m) or c < 2:
                continue
            mean, _ = bs.meancov_numpy(m, pc.to_points(m, X))
            mg = sc.belief_wrap_margin(m, X, mean)
            assert mg > sc.WRAP_MARGIN, (m, kind, c, seed, mg)
            least = min(least, mg)
    pair_sets = [(sc.kld_pairs(N), 300 + N) for N in sc.KLD_SIZES] + [(sc.mixed_pairs(40, 200, 61), 62)]
    for pairs, seed in pair_sets:
        for (m, _, _), (A, B) in zip(pairs, sc.pair_clouds(pairs, seed)):
            mg = sc.pair_wrap_margin(m, A, B)
            assert mg > sc.WRAP_MARGIN, (m, seed, mg)
            least = min(least, mg)
    print("least wrap margin", least)
