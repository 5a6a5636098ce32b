"""-m gpu: belief queries on the device (nbp_run_evaluate / nbp_kde_evaluate / nbp_run_mmd / nbp_kde_mmd, csrc/nbp_query.h) through
the C ABI and through the mirror, held to the criteria of tests/query_cases.py: densities within 1e-12 relative (+ 1e-300) of
the exact sums of density_numpy, mmd values within 1e-12 absolute of mmd_numpy, exact zeros and bit-equalities where the
definition promises them.

Clouds come from ppe_cases.cloud; bandwidths are fitted with nbp_run_bandwidth where a belief holds more than two points and
is not all-identical, and set by hand otherwise."""
import ctypes as C

import numpy as np
import pytest

import ppe_cases as pc
import query_cases as qc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
bq = iif.beliefquery
KINDS = ("gaussian", "across_pi", "around_circle", "identical")


def _load(be, items, seed, first_slot=0):
    """items = [(manifold, cloud kind, count)] -> slot first_slot + i holds belief i; returns (slots, manifolds, [(X, bw)]) with
    the tangent coordinates and bandwidths as read back from the slots"""
    rng = np.random.default_rng(seed)
    slots, mans = list(range(first_slot, first_slot + len(items))), [m for m, _, _ in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, pc.cloud(kind, m, c, rng)), pc.hand_bandwidth(m), None) for m, kind, c in items])
    fit = [i for i, (m, kind, c) in enumerate(items) if kind != "identical" and c > 2]
    if fit:
        be.run_bandwidth([slots[i] for i in fit], [mans[i] for i in fit])
    back = be.beliefs_read(slots, mans)
    for (pts, bw, _), (m, kind, c) in zip(back, items):
        assert len(pts) == c
    return slots, mans, [(coords(m, pts), bw) for (pts, bw, _), m in zip(back, mans)]


def _evaluate_and_check(be, items, slots, mans, beliefs, counts, seed):
    rng = np.random.default_rng(seed)
    Q = [qc.make_queries(m, X, bw, nq, rng) for m, (X, bw), nq in zip(mans, beliefs, counts)]
    dens = be.run_evaluate(slots, mans, Q)
    for i, (m, kind, c) in enumerate(items):
        qc.check_density(m, beliefs[i][0], beliefs[i][1], Q[i], dens[i], f"[{i}] manifold {m} {kind} c={c} N={be.N}")
    return Q, dens


@pytest.mark.parametrize("N", [64, 65, 200, 512])
def test_density_every_manifold_and_cloud_at_full_count(hip_backend, N):
    """query counts 0, 1, 4 and one more than a tile, mixed with the manifolds in ONE call"""
    items = [(m, kind, N) for m in qc.MANIFOLDS for kind in KINDS]
    counts = [(0, 1, 4, qc.TILE + 1)[(i + i // 4) % 4] for i in range(len(items))]
    assert {(m, q) for (m, _, _), q in zip(items, counts)} == {(m, q) for m in qc.MANIFOLDS for q in (0, 1, 4, qc.TILE + 1)}
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = _load(be, items, 300 + N)
        _evaluate_and_check(be, items, slots, mans, beliefs, counts, 400 + N)
    finally:
        be.close()


def test_density_counts_below_the_context_size(hip_backend):
    items = [(m, kind, c) for m in qc.MANIFOLDS for c in (1, 2, 63, 150) for kind in ("gaussian", "across_pi")]
    counts = [(qc.TILE + 1, 4, 1, 0, 4)[i % 5] for i in range(len(items))]
    be = hip_backend(200, len(items))
    try:
        slots, mans, beliefs = _load(be, items, 307)
        _evaluate_and_check(be, items, slots, mans, beliefs, counts, 308)
    finally:
        be.close()


def test_density_at_own_points_is_the_ppe_density_normalised(hip_backend):
    N = 200
    items = [(m, kind, c) for m in qc.MANIFOLDS for kind, c in (("gaussian", N), ("across_pi", 150))]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = _load(be, items, 311)
        dens = be.run_evaluate(slots, mans, [X for X, _ in beliefs])
        for i, (m, kind, c) in enumerate(items):
            X, bw = beliefs[i]
            p = iif.ppe.kde_density(m, X, bw)
            got = dens[i] * (c * np.prod(np.sqrt(2 * np.pi) * bw))
            print(f"[{i}] manifold {m} {kind}: max |dens norm - p_i| / p_i = {np.max(np.abs(got - p) / p):.3e}")
            assert np.all(np.abs(got - p) <= qc.DENS_RTOL * p + qc.DENS_ATOL), (i, got, p)
    finally:
        be.close()


def test_density_of_a_query_alone_is_its_value_in_a_batch(hip_backend):
    N = 200
    items = [(m, "gaussian", c) for m in qc.MANIFOLDS for c in (N, 63)]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = _load(be, items, 313)
        rng = np.random.default_rng(314)
        Q = [qc.make_queries(m, X, bw, qc.TILE + 1, rng) for m, (X, bw) in zip(mans, beliefs)]
        batch = be.run_evaluate(slots, mans, Q)
        again = be.run_evaluate(slots, mans, Q)
        for i in range(len(items)):
            assert np.array_equal(batch[i], again[i])
            for k in (0, 1, 5, qc.TILE - 1, qc.TILE):  # the last one is the second tile's only query
                alone = be.run_evaluate([slots[i]], [mans[i]], [Q[i][k:k + 1]])[0]
                assert np.array_equal(alone, batch[i][k:k + 1]), (i, k, alone, batch[i][k])
        # the host-buffer form of belief 3 (Euclid(2), 63 points) stages through slot 0, which nothing reads afterwards
        pts, bw, _ = be.beliefs_read([slots[3]], [mans[3]])[0]
        assert np.array_equal(be.kde_evaluate(mans[3], pts, bw, Q[3]), batch[3])
    finally:
        be.close()


def test_density_bad_bandwidth_gives_nan(hip_backend):
    N = 200
    items = [(m, "gaussian", c) for m in qc.MANIFOLDS for c in (N, 63)]
    be = hip_backend(N, len(items) + 1)
    rng = np.random.default_rng(317)
    try:
        slots, mans = list(range(len(items))), [m for m, _, _ in items]
        good = len(items)  # one healthy belief travels with them
        for k, bad in enumerate((0.0, np.nan, np.inf, -1.0)):
            bws = []
            for m in mans:
                bw = pc.hand_bandwidth(m).copy()
                bw[k % len(bw)] = bad
                bws.append(bw)
            Xs = [pc.cloud(kind, m, c, rng) for m, kind, c in items]
            G = pc.cloud("gaussian", abi.EUCLID2, 63, rng)
            be.beliefs_write(slots + [good], mans + [abi.EUCLID2],
                             [(pc.to_points(m, X), bws[i], None) for i, (m, X) in enumerate(zip(mans, Xs))] + [(G, [0.3, 0.3], None)])
            dens = be.run_evaluate(slots + [good], mans + [abi.EUCLID2], [X[:5] for X in Xs] + [G[:3]])
            for i in range(len(items)):
                assert dens[i].shape == (5,) and np.isnan(dens[i]).all(), (bad, i, dens[i])
            assert np.isfinite(dens[-1]).all() and np.all(dens[-1] > 0)
    finally:
        be.close()


def _pairs(N):
    """(cloud kind a, count a, cloud kind b, count b): overlapping, far apart, across +-pi on both sides, unequal counts"""
    return [("gaussian", N, "gaussian", N), ("gaussian", N, "far", N), ("gaussian", N, "across_pi", N), ("across_pi", N, "across_pi", N),
            ("around_circle", N, "two_cluster", N), ("gaussian", N, "gaussian", min(73, N)), ("gaussian", 1, "across_pi", min(150, N))]


def _pair_cloud(kind, m, c, rng):
    if kind != "far":
        return pc.cloud(kind, m, c, rng)
    x = pc.cloud("gaussian", m, c, rng)  # 25 away along the first coordinate; on the circle: on the other side
    x[:, 0] = pc.wrap(x[:, 0] + np.pi) if 0 in pc.circular_coords(m) else x[:, 0] + 25.0
    return x


def _load_pairs(be, pairs_m, seed):
    """pairs_m = [(manifold, kind a, count a, kind b, count b)] -> a in slot 2 i, b in slot 2 i + 1; returns (slots a, slots b,
    manifolds, tangent coordinates of every a and of every b as read back)"""
    rng = np.random.default_rng(seed)
    mans = [m for m, *_ in pairs_m for _ in range(2)]
    slots = list(range(len(mans)))
    X = [_pair_cloud(k, m, c, rng) for m, ka, ca, kb, cb in pairs_m for k, c in ((ka, ca), (kb, cb))]
    be.beliefs_write(slots, mans, [(pc.to_points(m, x), pc.hand_bandwidth(m), None) for m, x in zip(mans, X)])
    X = [coords(m, pts) for (pts, _, _), m in zip(be.beliefs_read(slots, mans), mans)]
    return slots[0::2], slots[1::2], mans[0::2], X[0::2], X[1::2]


@pytest.mark.parametrize("N", [64, 65, 200, 512])
def test_mmd_every_manifold(hip_backend, N):
    pairs_m = [(m,) + p for m in qc.MANIFOLDS for p in _pairs(N)]
    be = hip_backend(N, 2 * len(pairs_m))
    try:
        sa, sb, mans, XA, XB = _load_pairs(be, pairs_m, 500 + N)
        for sigma in (0.001, 1.0):
            dev = be.run_mmd(sa, sb, mans, sigma)
            for i, pm in enumerate(pairs_m):
                qc.check_mmd(mans[i], XA[i], XB[i], sigma, dev[i], f"[{i}] {pm} N={N}")
            assert np.all(be.run_mmd(sa, sa, mans, sigma) == 0.0) and np.all(be.run_mmd(sb, sb, mans, sigma) == 0.0)
    finally:
        be.close()


def test_mmd_batch_of_40_mixed_pairs_and_exact_zeros(hip_backend):
    N = 200
    rng = np.random.default_rng(521)
    kinds = ("gaussian", "two_cluster", "around_circle", "across_pi", "identical")
    pairs_m = [(qc.MANIFOLDS[rng.integers(5)], kinds[rng.integers(5)], int(rng.choice([N, N, 150, 73, 2, 1])),
                kinds[rng.integers(5)], int(rng.choice([N, N, 150, 73, 2, 1]))) for _ in range(40)]
    be = hip_backend(N, 2 * len(pairs_m))
    try:
        sa, sb, mans, XA, XB = _load_pairs(be, pairs_m, 522)
        dev = be.run_mmd(sa, sb, mans, 0.05)
        assert dev.tobytes() == be.run_mmd(sa, sb, mans, 0.05).tobytes()
        for i, pm in enumerate(pairs_m):
            qc.check_mmd(mans[i], XA[i], XB[i], 0.05, dev[i], f"[{i}] {pm}")
            assert be.run_mmd([sa[i]], [sb[i]], [mans[i]], 0.05)[0] == dev[i]
        # two slots written with the same points: exactly zero, whatever the count
        back = be.beliefs_read(sa, mans)
        be.beliefs_write(sb, mans, [(p, [1.0, 2.0, 3.0][:len(bw)], None) for p, bw, _ in back])
        for sigma in (0.001, 0.05, 1.0):
            assert np.all(be.run_mmd(sa, sb, mans, sigma) == 0.0)
    finally:
        be.close()


def test_kde_mmd_is_run_mmd_bit_for_bit(hip_backend):
    N = 200
    pairs_m = [(m,) + p for m in qc.MANIFOLDS for p in _pairs(N)[1:]]
    be = hip_backend(N, 2 * len(pairs_m) + 2)
    try:
        rng = np.random.default_rng(531)
        A = [pc.to_points(m, _pair_cloud(ka, m, ca, rng)) for m, ka, ca, kb, cb in pairs_m]
        B = [pc.to_points(m, _pair_cloud(kb, m, cb, rng)) for m, ka, ca, kb, cb in pairs_m]
        mans = [p[0] for p in pairs_m]
        sa, sb = list(range(2, 2 + len(A))), list(range(2 + len(A), 2 + 2 * len(A)))  # slots 0 and 1 are kde_mmd's
        be.beliefs_write(sa + sb, mans + mans, [(p, pc.hand_bandwidth(m), None) for p, m in zip(A + B, mans + mans)])
        for sigma in (0.001, 1.0):
            res = be.run_mmd(sa, sb, mans, sigma)
            for i, m in enumerate(mans):
                assert be.kde_mmd(m, A[i], B[i], sigma) == res[i], (i, pairs_m[i])
                assert be.kde_mmd(m, A[i], A[i], sigma) == 0.0
    finally:
        be.close()


def test_mirror_equals_the_abi_calls_and_numpy():
    fg, fg2, fg3 = qc.chain6(5), qc.chain6(5), qc.chain6(5)
    iif.solveTree(fg, backend=iif.HipBackend, seed=71)
    iif.solveTree(fg2, backend=iif.HipBackend, seed=72)
    iif.solveTree(fg3, backend=iif.HipBackend, seed=71)
    labels = [f"x{i}" for i in range(6)]
    v = fg.getVariable("x5")
    pts = np.concatenate([v.val[:7], [[4.0], [5.0], [5.3], [9.0]]])
    be = iif.HipBackend(len(v.val), 12)
    try:
        b = iif.getBelief(fg, "x5")
        got = b(pts, backend=be)
        assert np.array_equal(got, be.kde_evaluate(abi.EUCLID1, v.val, v.bw, pts))
        assert np.array_equal(got, b(pts, backend=iif.HipBackend))  # a backend of its own
        qc.check_density(abi.EUCLID1, v.val, v.bw, pts, got, "getBelief(fg, x5)")
        names, vals = iif.mmdVariables(fg, fg2, backend=be)
        assert names == labels
        # what mmdVariables did, by hand: A in slots 0 .. 5, B in 6 .. 11, one run_mmd
        mans = [abi.EUCLID1] * 6
        be.beliefs_write(list(range(12)), mans + mans, [(g.getVal(l), g.getVariable(l).bw, None) for g in (fg, fg2) for l in labels])
        assert np.array_equal(vals, be.run_mmd(list(range(6)), list(range(6, 12)), mans, 0.001))
        for i, l in enumerate(labels):
            qc.check_mmd(abi.EUCLID1, fg.getVal(l), fg2.getVal(l), 0.001, vals[i], l)
            assert vals[i] == iif.mmd(fg.getVal(l), iif.getBelief(fg2, l), iif.ContinuousScalar, backend=be)
            assert vals[i] > 0
        # the same seed gives the same particles: 0.0 everywhere
        for l in labels:
            assert np.array_equal(fg.getVal(l), fg3.getVal(l))
        assert np.all(iif.mmdVariables(fg, fg3, backend=be)[1] == 0.0)
        assert np.all(iif.mmdVariables(fg, fg3, backend=iif.HipBackend)[1] == 0.0)
        assert iif.isapproxBeliefs(iif.getBelief(fg, "x5"), iif.getBelief(fg3, "x5"), iif.ContinuousScalar, backend=be)
    finally:
        be.close()


def test_argument_errors_behave_as_run_ppes_do(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp = C.POINTER(C.c_double)
    try:
        rng = np.random.default_rng(541)
        X = pc.cloud("gaussian", abi.EUCLID2, 64, rng)
        be.slot_write(0, abi.EUCLID2, X, [0.3, 0.3])
        be.slot_write(1, abi.EUCLID2, X + 1.0, [0.3, 0.3])
        for bad in (-1, 4):
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_evaluate([bad], [abi.EUCLID2], [X[:2]])
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_mmd([bad], [0], [abi.EUCLID2])
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_mmd([0], [bad], [abi.EUCLID2])
        for bad in (0, 6):
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_evaluate([0], [bad], [X[:2]])
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_mmd([0], [1], [bad])
        for bad in (-0.5, np.nan, np.inf):
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_mmd([0], [1], [abi.EUCLID2], bad)
            with pytest.raises(iif.NbpError, match="-1"):
                be.kde_mmd(abi.EUCLID2, X, X, bad)
        one, two, man = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1), (C.c_int32 * 1)(abi.EUCLID2)
        qf, q, out = (C.c_int32 * 2)(0, 2), (C.c_double * 6)(), (C.c_double * 2)()
        assert lib.nbp_run_evaluate(ctx, one, man, 1, qf, q, out) == 0
        assert lib.nbp_run_evaluate(None, one, man, 1, qf, q, out) == -1
        assert lib.nbp_run_evaluate(ctx, None, man, 1, qf, q, out) == -1
        assert lib.nbp_run_evaluate(ctx, one, None, 1, qf, q, out) == -1
        assert lib.nbp_run_evaluate(ctx, one, man, 1, None, q, out) == -1
        assert lib.nbp_run_evaluate(ctx, one, man, 1, qf, None, out) == -1
        assert lib.nbp_run_evaluate(ctx, one, man, 1, qf, q, None) == -1
        assert lib.nbp_run_evaluate(ctx, None, None, 0, None, None, None) == 0       # n = 0 is NBP_OK
        assert lib.nbp_run_evaluate(ctx, one, man, 1, (C.c_int32 * 2)(0, 0), None, None) == 0  # a belief with no query
        assert lib.nbp_run_evaluate(ctx, one, man, 1, (C.c_int32 * 2)(1, 2), q, out) == -1     # q_first[0] != 0
        assert lib.nbp_run_evaluate(ctx, (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(2, 2), 2, (C.c_int32 * 3)(0, 2, 1), q, out) == -1
        assert b"q_first" in lib.nbp_last_error()
        assert lib.nbp_run_mmd(ctx, one, two, man, 1, 0.001, out) == 0
        assert lib.nbp_run_mmd(None, one, two, man, 1, 0.001, out) == -1
        assert lib.nbp_run_mmd(ctx, None, two, man, 1, 0.001, out) == -1
        assert lib.nbp_run_mmd(ctx, one, None, man, 1, 0.001, out) == -1
        assert lib.nbp_run_mmd(ctx, one, two, None, 1, 0.001, out) == -1
        assert lib.nbp_run_mmd(ctx, one, two, man, 1, 0.001, None) == -1
        assert lib.nbp_run_mmd(ctx, None, None, None, 0, 0.001, None) == 0
        assert lib.nbp_run_mmd(ctx, one, one, man, 1, 0.001, out) == 0 and out[0] == 0.0     # the same slot on both sides
        pts, bw = np.ascontiguousarray(X), np.array([0.3, 0.3])
        P, B = pts.ctypes.data_as(dp), bw.ctypes.data_as(dp)
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 64, B, q, 2, out) == 0
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, None, 64, B, q, 2, out) == -1
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 64, None, q, 2, out) == -1
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 64, B, None, 2, out) == -1
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 64, B, q, 2, None) == -1
        assert lib.nbp_kde_evaluate(ctx, 9, P, 64, B, q, 2, out) == -1
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 0, B, q, 2, out) == -1               # an empty belief
        assert lib.nbp_kde_evaluate(ctx, abi.EUCLID2, P, 64, B, None, 0, None) == 0           # no query
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, P, 64, P, 30, 0.001, out) == 0
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, None, 64, P, 30, 0.001, out) == -1
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, P, 64, None, 30, 0.001, out) == -1
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, P, 64, P, 30, 0.001, None) == -1
        assert lib.nbp_kde_mmd(ctx, 0, P, 64, P, 30, 0.001, out) == -1
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, P, 0, P, 30, 0.001, out) == -1               # an empty belief, either side
        assert lib.nbp_kde_mmd(ctx, abi.EUCLID2, P, 64, P, 0, 0.001, out) == -1
        small = hip_backend(64, 1)
        try:
            with pytest.raises(iif.NbpError, match="-4"):
                small.kde_mmd(abi.EUCLID2, X, X)  # stages through slots 0 and 1
            assert len(small.kde_evaluate(abi.EUCLID2, X, [0.3, 0.3], X[:3])) == 3
        finally:
            small.close()
        # the context stays usable
        be.slot_write(0, abi.EUCLID2, X, [0.3, 0.3])
        be.slot_write(1, abi.EUCLID2, X + 1.0, [0.3, 0.3])
        d = be.run_evaluate([0], [abi.EUCLID2], [X[:3]])[0]
        assert np.isfinite(d).all() and np.all(d > 0) and be.run_mmd([0], [1], [abi.EUCLID2], 1.0)[0] > 0
    finally:
        be.close()
