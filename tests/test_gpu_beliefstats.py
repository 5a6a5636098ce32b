"""-m gpu: belief statistics on the device (nbp_run_meancov / nbp_kde_meancov / nbp_run_kld / nbp_kde_kld, csrc/nbp_stats.h) through
the C ABI and through the mirror, held to the criteria of tests/stats_cases.py: the mean to run_ppe's bits, the covariance to the
numpy restatement about the device's mean within c + 4 roundings, the kld to the numpy restatement within 1e-12 of its terms.

Beliefs of fewer than three points carry a bandwidth set by hand (a leave-one-out fit has nothing to leave out of one point); so
do the all-identical ones; every other bandwidth of the kld tests comes from nbp_run_bandwidth."""
import ctypes as C

import numpy as np
import pytest

import ppe_cases as pc
import stats_cases as sc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
bs = iif.beliefstats


def _check_meancov(be, items, slots, mans, out):
    mean, cov = out
    assert mean.tobytes() == be.run_ppe(slots, mans)[0].tobytes()
    back = be.beliefs_read(slots, mans)
    for i, (m, kind, c) in enumerate(items):
        assert len(back[i][0]) == c
        sc.check_cov(m, back[i][0], mean[i], cov[i], f"[{i}] manifold {m} {kind} c={c} N={be.N}")


@pytest.mark.parametrize("N", sc.FULL_COUNTS)
def test_meancov_every_manifold_and_cloud_at_full_count(hip_backend, N):
    items = sc.full_items(N)
    be = hip_backend(N, len(items))
    try:
        slots, mans = sc.load(be, items, 100 + N)
        _check_meancov(be, items, slots, mans, be.run_meancov(slots, mans))
    finally:
        be.close()


def test_meancov_counts_below_the_context_size(hip_backend):
    items = sc.below_items()
    be = hip_backend(200, len(items))
    try:
        slots, mans = sc.load(be, items, 7)
        mean, cov = be.run_meancov(slots, mans)
        _check_meancov(be, items, slots, mans, (mean, cov))
        back = be.beliefs_read(slots, mans)
        for i, (m, kind, c) in enumerate(items):
            D = abi.MANIFOLD_DIM[m]
            if c == 1:  # NaN covariance, and the mean is the point
                assert np.isnan(cov[i, :D, :D]).all(), (i, cov[i])
                d = mean[i, :D] - coords(m, back[i][0])[0]
                assert np.all(d[:2] == 0) and (np.all(d == 0) if m != abi.SE2 else abs(d[2]) <= 1e-15), (i, mean[i], back[i][0])
            elif kind == "identical":  # (check_cov has held it to the bound: A and B are ~0 here)
                assert np.abs(cov[i]).max() <= 1e-28, (i, cov[i])
    finally:
        be.close()


def test_meancov_batch_of_300_is_deterministic(hip_backend):
    """more workgroups than the chip has CUs, manifolds and counts mixed in one launch"""
    items = sc.batch_items(300, 200, 21)
    be = hip_backend(200, len(items))
    try:
        slots, mans = sc.load(be, items, 22)
        a, b = be.run_meancov(slots, mans), be.run_meancov(slots, mans)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        _check_meancov(be, items, slots, mans, a)
        for i in range(len(items)):
            one = be.run_meancov([slots[i]], [mans[i]])
            for x, y in zip(a, one):
                assert x[i].tobytes() == y[0].tobytes(), (i, items[i])
    finally:
        be.close()


def test_kde_forms_equal_resident_forms(hip_backend):
    N = 200
    items = [(m, kind, c) for m in sc.MANIFOLDS for kind, c in (("gaussian", N), ("two_cluster", N), ("across_pi", 150), ("gaussian", 1))]
    be = hip_backend(N, len(items) + 2)
    try:
        Xs = sc.clouds(items, 41)
        slots, mans = list(range(2, len(items) + 2)), [m for m, _, _ in items]  # slots 0 and 1 are the staging slots
        pts = [pc.to_points(m, X) for m, X in zip(mans, Xs)]
        bws = [pc.hand_bandwidth(m) * (1 + 0.1 * (i % 3)) for i, m in enumerate(mans)]
        be.beliefs_write(slots, mans, [(p, h, None) for p, h in zip(pts, bws)])
        mean, cov = be.run_meancov(slots, mans)
        for i, m in enumerate(mans):
            D = abi.MANIFOLD_DIM[m]
            m1, c1 = be.kde_meancov(m, pts[i])
            assert m1.shape == (D,) and c1.shape == (D, D)
            assert m1.tobytes() == mean[i, :D].tobytes() and c1.tobytes() == np.ascontiguousarray(cov[i, :D, :D]).tobytes(), (i, items[i])
        pairs = [(i, j) for i in range(len(items)) for j in range(len(items)) if mans[i] == mans[j] and i != j]
        val, tm = be.run_kld([slots[i] for i, _ in pairs], [slots[j] for _, j in pairs], [mans[i] for i, _ in pairs], terms=True)
        for k, (i, j) in enumerate(pairs):
            v1, t1 = be.kde_kld(mans[i], pts[i], bws[i], pts[j], bws[j], terms=True)
            assert np.float64(v1).tobytes() == val[k].tobytes() and t1.tobytes() == tm[k].tobytes(), (i, j, v1, val[k])
            assert np.float64(be.kde_kld(mans[i], pts[i], bws[i], pts[j], bws[j])).tobytes() == val[k].tobytes()
    finally:
        be.close()


@pytest.mark.parametrize("N", sc.KLD_SIZES)
def test_kld_every_manifold(hip_backend, N):
    pairs = sc.kld_pairs(N)
    be = hip_backend(N, 2 * len(pairs))
    try:
        sa, sb, mans = sc.load_pairs(be, pairs, 300 + N)
        val, tm = be.run_kld(sa, sb, mans, terms=True)
        assert be.run_kld(sa, sb, mans).tobytes() == val.tobytes()
        print("worst |diff| / bound", sc.check_kld(be, sa, sb, mans, val, tm, f"N={N} "))
    finally:
        be.close()


def test_kld_exact_zeros(hip_backend):
    N = 200
    items = [(m, kind, c) for m in sc.MANIFOLDS for kind, c in (("gaussian", N), ("two_cluster", 150), ("across_pi", 63), ("gaussian", 1))]
    be = hip_backend(N, 2 * len(items))
    try:
        Xs = sc.clouds(items, 51)
        n, mans = len(items), [m for m, _, _ in items]
        bel = [(pc.to_points(m, X), pc.hand_bandwidth(m), None) for m, X in zip(mans, Xs)]
        a = list(range(n))
        be.beliefs_write(a, mans, bel)
        fit = [i for i, (m, kind, c) in enumerate(items) if c > 2]
        be.run_bandwidth(fit, [mans[i] for i in fit])
        bel = [(p, bw, None) for (p, _, _), (_, bw, _) in zip(bel, be.beliefs_read(a, mans))]  # the fitted bandwidths, as stored
        be.beliefs_write(list(range(2 * n)), mans + mans, bel + bel)  # slot n + i: a bit-identical copy of slot i
        for b in (a, [n + i for i in a]):
            val, tm = be.run_kld(a, b, mans, terms=True)
            assert val.tobytes() == np.zeros(n).tobytes(), val  # +0.0, every one
            assert np.isfinite(tm).all() and np.array_equal(tm[:, 0], tm[:, 1])
    finally:
        be.close()


@pytest.mark.parametrize("man", [abi.EUCLID1, abi.EUCLID2, abi.EUCLID3])
def test_kld_far_apart_is_finite(hip_backend, man):
    """b lies 1000 bandwidths from a in every coordinate.  A term of the density below exp(-700) enters as the clamp of
    exp_nonpos (~1e-304), not as 0 (nbp_query.h), so the density reaches exactly 0.0 where the normaliser c prod sqrt(2 pi) h_d
    carries it below the smallest subnormal: the bandwidths here are that large (the scale is free: the offset is counted in
    bandwidths).  The log-density is finite all the same, and the kld within the bound."""
    D = abi.MANIFOLD_DIM[man]
    h = np.full(D, (1e30, 1e15, 1e10)[D - 1])
    rng = np.random.default_rng(71 + D)
    A, B = h * rng.normal(size=(200, D)), h * rng.normal(size=(150, D)) + 1000 * h
    be = hip_backend(200, 2)
    try:
        be.beliefs_write([0, 1], [man, man], [(A, h, None), (B, h, None)])
        dens = be.run_evaluate([1], [man], [A])[0]
        print("densities of b at a's points: max", dens.max())
        assert dens.shape == (200,) and np.all(dens == 0.0), dens.max()
        val, tm = be.run_kld([0], [1], [man], terms=True)
        assert np.isfinite(val).all() and np.isfinite(tm).all() and val[0] > 4e5 * D
        sc.check_kld(be, [0], [1], [man], val, tm, "far apart ")
    finally:
        be.close()


def test_kld_terms_and_entropy(hip_backend):
    pairs = sc.mixed_pairs(12, 200, 81)
    be = hip_backend(200, 2 * len(pairs) + 2)
    try:
        sa, sb, mans = sc.load_pairs(be, pairs, 82, first_slot=2)  # (slots 0 and 1 are the staging slots of the host-buffer form)
        val, tm = be.run_kld(sa, sb, mans, terms=True)
        assert (tm[:, 0] - tm[:, 1]).tobytes() == val.tobytes()
        back = be.beliefs_read(sa, mans)
        for i, m in enumerate(mans):
            pts, bw, _ = back[i]
            ent = iif.entropy((pts, bw), m, backend=be)
            self_val, self_tm = be.run_kld([sa[i]], [sa[i]], [m], terms=True)
            assert self_tm[0, 0].tobytes() == tm[i, 0].tobytes()  # Eaa does not depend on b
            want = -bs.kld_terms_numpy(m, coords(m, pts), bw, coords(m, pts), bw)[0]
            assert abs(ent - want) <= sc.KLD_RTOL * (1 + 2 * abs(want)), (i, ent, want)
            if m != abi.SE2:  # (the host-buffer form writes the heading back through atan2: an ulp of theta)
                assert np.float64(ent).tobytes() == np.float64(-tm[i, 0]).tobytes(), (i, ent, tm[i, 0])
    finally:
        be.close()


def test_kld_batch_of_40_mixed_pairs(hip_backend):
    pairs = sc.mixed_pairs(40, 200, 61)
    be = hip_backend(200, 2 * len(pairs))
    try:
        sa, sb, mans = sc.load_pairs(be, pairs, 62)
        v1, t1 = be.run_kld(sa, sb, mans, terms=True)
        v2, t2 = be.run_kld(sa, sb, mans, terms=True)
        assert v1.tobytes() == v2.tobytes() and t1.tobytes() == t2.tobytes()
        sc.check_kld(be, sa, sb, mans, v1, t1, "batch ")
        for i in range(len(pairs)):
            v, t = be.run_kld([sa[i]], [sb[i]], [mans[i]], terms=True)
            assert v[0].tobytes() == v1[i].tobytes() and t[0].tobytes() == t1[i].tobytes(), (i, pairs[i])
    finally:
        be.close()


def test_kld_bad_bandwidth_gives_nan(hip_backend):
    """zero, NaN, inf or negative, in a or in b, each coordinate of the manifold in turn: NaN kld, NaN terms; the covariance of
    the same slots does not read the bandwidth"""
    N = 65
    cases = [(m, side, d, bad) for m in sc.MANIFOLDS for side in (0, 1) for d in range(abi.MANIFOLD_DIM[m])
             for bad in (0.0, np.nan, np.inf, -1.0)]
    be = hip_backend(N, 2 * len(cases))
    try:
        items = [(m, "gaussian", (N, 63)[k % 2]) for m, _, _, _ in cases for k in range(2)]
        Xs = sc.clouds(items, 91)
        slots, mans = list(range(len(items))), [m for m, _, _ in items]
        good = [(pc.to_points(m, X), pc.hand_bandwidth(m), None) for m, X in zip(mans, Xs)]
        be.beliefs_write(slots, mans, good)
        sa, sb, pm = slots[0::2], slots[1::2], mans[0::2]
        val0 = be.run_kld(sa, sb, pm)
        assert np.isfinite(val0).all()
        mc0 = be.run_meancov(slots, mans)
        spoiled = list(good)
        for i, (m, side, d, bad) in enumerate(cases):
            bw = pc.hand_bandwidth(m).copy()
            bw[d] = bad
            spoiled[2 * i + side] = (good[2 * i + side][0], bw, None)
        be.beliefs_write(slots, mans, spoiled)
        val, tm = be.run_kld(sa, sb, pm, terms=True)
        assert np.isnan(val).all() and np.isnan(tm).all(), [c for c, v in zip(cases, val) if not np.isnan(v)]
        mc = be.run_meancov(slots, mans)
        assert mc[0].tobytes() == mc0[0].tobytes() and mc[1].tobytes() == mc0[1].tobytes()
    finally:
        be.close()


def test_argument_errors_behave_as_run_ppes_do(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp = C.POINTER(C.c_double)
    try:
        rng = np.random.default_rng(51)
        for s in (0, 1):
            be.slot_write(s, abi.EUCLID2, pc.cloud("gaussian", abi.EUCLID2, 64, rng), [0.3, 0.3])
        for bad in (-1, 4):
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_meancov([bad], [abi.EUCLID2])
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_kld([bad], [0], [abi.EUCLID2])
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_kld([0], [bad], [abi.EUCLID2])
        for bad in (0, 6):
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_meancov([0], [bad])
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_kld([0], [1], [bad])
        one, two, man = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1), (C.c_int32 * 1)(abi.EUCLID2)
        m3, c9, k1, t2 = (C.c_double * 3)(), (C.c_double * 9)(), (C.c_double * 1)(), (C.c_double * 2)()
        assert lib.nbp_run_meancov(ctx, None, man, 1, m3, c9) == -1
        assert lib.nbp_run_meancov(ctx, one, None, 1, m3, c9) == -1
        assert lib.nbp_run_meancov(ctx, one, man, 1, None, c9) == -1
        assert lib.nbp_run_meancov(ctx, one, man, 1, m3, None) == -1
        assert lib.nbp_run_meancov(None, one, man, 1, m3, c9) == -1
        assert lib.nbp_run_meancov(ctx, None, None, 0, None, None) == 0  # n = 0 is NBP_OK
        assert lib.nbp_run_meancov(ctx, one, man, 1, m3, c9) == 0
        assert lib.nbp_run_kld(ctx, None, two, man, 1, k1, t2) == -1
        assert lib.nbp_run_kld(ctx, one, None, man, 1, k1, t2) == -1
        assert lib.nbp_run_kld(ctx, one, two, None, 1, k1, t2) == -1
        assert lib.nbp_run_kld(ctx, one, two, man, 1, None, t2) == -1
        assert lib.nbp_run_kld(None, one, two, man, 1, k1, t2) == -1
        assert lib.nbp_run_kld(ctx, None, None, None, 0, None, None) == 0
        assert lib.nbp_run_kld(ctx, one, two, man, 1, k1, None) == 0  # the terms are optional
        pts = np.ascontiguousarray(pc.cloud("gaussian", abi.EUCLID2, 64, rng))
        bw = np.array([0.3, 0.3])
        P, H = pts.ctypes.data_as(dp), bw.ctypes.data_as(dp)
        assert lib.nbp_kde_meancov(ctx, abi.EUCLID2, None, 64, m3, c9) == -1
        assert lib.nbp_kde_meancov(ctx, abi.EUCLID2, P, 64, None, c9) == -1
        assert lib.nbp_kde_meancov(ctx, 9, P, 64, m3, c9) == -1
        assert lib.nbp_kde_meancov(ctx, abi.EUCLID2, P, 0, m3, c9) == -1
        assert lib.nbp_kde_meancov(ctx, abi.EUCLID2, P, 64, m3, c9) == 0
        assert lib.nbp_kde_kld(ctx, abi.EUCLID2, None, 64, H, P, 64, H, k1, t2) == -1
        assert lib.nbp_kde_kld(ctx, abi.EUCLID2, P, 64, None, P, 64, H, k1, t2) == -1
        assert lib.nbp_kde_kld(ctx, abi.EUCLID2, P, 64, H, P, 64, None, k1, t2) == -1
        assert lib.nbp_kde_kld(ctx, abi.EUCLID2, P, 64, H, P, 64, H, None, t2) == -1
        assert lib.nbp_kde_kld(ctx, 9, P, 64, H, P, 64, H, k1, t2) == -1
        assert lib.nbp_kde_kld(ctx, abi.EUCLID2, P, 64, H, P, 64, H, k1, None) == 0 and k1[0] == 0.0
        # the context stays usable
        mean, cov = be.run_meancov([0], [abi.EUCLID2])
        assert np.isfinite(mean).all() and np.isfinite(cov).all() and cov[0, 0, 0] > 0
        assert be.run_kld([0], [0], [abi.EUCLID2])[0] == 0.0
    finally:
        be.close()


def _chain(graph):
    fg = iif.initfg(iif.SolverParams(N=100))
    if graph == "euclid1_chain6":
        n = 6
        for i in range(n):
            iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
        iif.addFactor(fg, ["x0"], iif.Prior(iif.Normal(0.0, 0.1)))
        for i in range(n - 1):
            iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    else:  # the graph of test/testCircular.jl:7-29
        n = 5
        for i in range(n):
            iif.addVariable(fg, f"x{i}", iif.Circular)
        iif.addFactor(fg, ["x0"], iif.PriorCircular(iif.Normal(0.0, 0.1)))
        for i in range(n - 1):
            iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.CircularCircular(iif.Normal(1.0, 0.1)))
    return fg, n


@pytest.mark.parametrize("graph", ["euclid1_chain6", "circular_chain5"])
def test_mirror_equals_abi_and_numpy(hip_backend, graph):
    fg, n = _chain(graph)
    iif.solveTree(fg, backend=iif.HipBackend, seed=61)
    be = hip_backend(100, 2)
    try:
        allv = iif.calcMeanCovarAll(fg, backend=iif.HipBackend)
        for i in range(n):
            v = fg.getVariable(f"x{i}")
            m = v.varType.manifold
            mu, Sig = iif.calcMeanCovar(fg, f"x{i}", backend=iif.HipBackend)
            m1, c1 = be.kde_meancov(m, v.val)
            assert mu.tobytes() == m1.tobytes() and Sig.tobytes() == c1.tobytes()
            assert allv[f"x{i}"][0].tobytes() == mu.tobytes() and allv[f"x{i}"][1].tobytes() == Sig.tobytes()
            mean3, cov3 = np.zeros(3), np.zeros((3, 3))
            mean3[:1], cov3[:1, :1] = mu, Sig
            sc.check_cov(m, v.val, mean3, cov3, f"{graph} x{i}")
            assert abs(pc.wrap(mu[0] - i) if graph == "circular_chain5" else mu[0] - i) < 0.5 and 0 < Sig[0, 0] < 1.0, (i, mu, Sig)
        b0, b1 = iif.getBelief(fg, "x0"), iif.getBelief(fg, "x1")
        m = b0.manifold
        k = iif.kld(b0, b1, fg.getVariable("x0").varType, backend=iif.HipBackend)
        k1, t1 = be.kde_kld(m, b0.pts, b0.bw, b1.pts, b1.bw, terms=True)
        assert np.float64(k).tobytes() == np.float64(k1).tobytes()
        assert sc.pair_wrap_margin(m, b0.pts, b1.pts) > sc.WRAP_MARGIN
        eaa, eab = bs.kld_terms_numpy(m, b0.pts, b0.bw, b1.pts, b1.bw)
        print(f"{graph}: kld(x0, x1) = {k} (numpy {eaa - eab}), entropy(x0) = {-t1[0]}")
        assert abs(k - (eaa - eab)) <= sc.KLD_RTOL * (1 + abs(eaa) + abs(eab))
        assert np.float64(iif.entropy(b0, m, backend=be)).tobytes() == np.float64(-t1[0]).tobytes()
    finally:
        be.close()


def test_session_calcmeancovar_moves_no_belief(hip_backend):
    fg = iif.generateChainEuclid(8, vardims=2, priorEvery=4, N=100)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=5)
        before = {k: ses.stats[k] for k in ("uploads", "readbacks")}
        got = ses.calcMeanCovar()
        assert {k: ses.stats[k] for k in before} == before
        assert list(got) == fg.ls() and len(got) == 8
        for v in fg.ls():
            mu, Sig = iif.calcMeanCovar(fg, v, backend=hip_backend)
            assert mu.shape == (2,) and Sig.shape == (2, 2)
            assert got[v][0].tobytes() == mu.tobytes() and got[v][1].tobytes() == Sig.tobytes(), v
        one = ses.calcMeanCovar(["x3"])
        assert list(one) == ["x3"] and one["x3"][1].tobytes() == got["x3"][1].tobytes()
        assert {k: ses.stats[k] for k in before} == before
        # an edit on the host: the belief goes up once, by the session's own path, and the answer is the new belief's
        rng = np.random.default_rng(6)
        new = rng.normal(2.0, 0.25, (100, 2))
        iif.setValKDE(fg, "x3", new, [0.1, 0.1])
        one = ses.calcMeanCovar(["x3"])
        assert ses.stats["uploads"] == before["uploads"] + 1 and ses.stats["readbacks"] == before["readbacks"]
        mean3, cov3 = np.zeros(3), np.zeros((3, 3))
        mean3[:2], cov3[:2, :2] = one["x3"]
        sc.check_cov(abi.EUCLID2, new, mean3, cov3, "x3 after setValKDE")
        assert np.abs(one["x3"][1] - np.cov(new.T)).max() < 1e-12
        ses.calcMeanCovar()
        assert ses.stats["uploads"] == before["uploads"] + 1  # resident now
