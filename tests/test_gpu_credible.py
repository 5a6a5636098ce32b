"""-m gpu: credible regions on the device (nbp_run_credible / nbp_kde_credible, csrc/nbp_credible.h) through the C ABI and through the
mirror, held to the criteria of tests/credible_cases.py: the leave-one-out log densities and the queries' log densities to the numpy
restatement within 1e-12 (1 + |l|), the order, the levels and every count exactly on the device's own values, the quantiles to the
hand-written formula bit for bit (the SE(2) heading within the allowance of its round trip), the mean to run_ppe's bits.

The bandwidths are set by hand (tests/test_credible.py walks the same beliefs on the CPU and asserts the conditions under which the
device's counts are compared with numpy's)."""
import ctypes as C

import numpy as np
import pytest

import credible_cases as cc
import ppe_cases as pc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
cr = iif.credible


def _load(be, items, nq, seed, first_slot=0):
    bel = cc.beliefs(items, nq, seed)
    slots, mans = list(range(first_slot, first_slot + len(items))), [m for m, _, _ in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), h, None) for m, (X, h, _) in zip(mans, bel)])
    return slots, mans, [Q for _, _, Q in bel]


def _check(be, items, masks, slots, mans, Qs, out, what=""):
    recs, ld, od, qrecs, first = out
    assert recs["mean"].tobytes() == be.run_ppe(slots, mans)[0].tobytes()
    back = be.beliefs_read(slots, mans)
    worst = 0.0
    for i, (m, kind, c) in enumerate(items):
        assert len(back[i][0]) == c
        worst = max(worst, cc.check_belief(m, masks[i], back[i][0], back[i][1], cc.MASS, cc.PROBS, recs[i], ld[i], od[i], Qs[i],
                                           qrecs[first[i]:first[i + 1]], f"{what}[{i}] manifold {m} {kind} c={c} mask={masks[i]} N={be.N}",
                                           ties=cc.exact_ties(kind, c)))
    print(f"{what}: {len(items)} beliefs, worst |dev - ref| / bound {worst:.3f}")
    return worst


def _scenario(hip_backend, name):
    N, items, masks, nq, seed = cc.scenario(name)
    be = hip_backend(N, len(items))
    slots, mans, Qs = _load(be, items, nq, seed)
    return be, items, masks, slots, mans, Qs


@pytest.mark.parametrize("N", cc.FULL_COUNTS)
def test_every_manifold_and_cloud_at_full_count(hip_backend, N):
    be, items, masks, slots, mans, Qs = _scenario(hip_backend, f"full{N}")
    try:
        _check(be, items, masks, slots, mans, Qs, be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs), f"N={N}")
    finally:
        be.close()


def test_counts_below_the_context_size(hip_backend):
    """the padding boundaries of the sort (63 / 64 / 65, 127 / 128 / 129 in a sort of 256), and the counts without levels"""
    be, items, masks, slots, mans, Qs = _scenario(hip_backend, "below")
    try:
        out = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        _check(be, items, masks, slots, mans, Qs, out, "below")
        recs, ld, od, qrecs, first = out
        back = be.beliefs_read(slots, mans)
        for i, (m, kind, c) in enumerate(items):
            if c == 1:  # no level, order = {0}, every quantile is the point
                D = abi.MANIFOLD_DIM[m]
                x = coords(m, back[i][0])[0]
                assert od[i, 0] == 0 and np.isnan(recs["log_level"][i, :len(cc.MASS)]).all(), (i, od[i, :2], recs[i])
                d = recs["quant"][i, :D, :len(cc.PROBS)] - x[:, None]
                assert np.all(d[:2] == 0) and (np.all(d == 0) if m != abi.SE2 else np.abs(d[2]).max() <= 1e-15), (i, recs["quant"][i], x)
    finally:
        be.close()


def test_every_mask_of_every_manifold(hip_backend):
    be, items, masks, slots, mans, Qs = _scenario(hip_backend, "masks")
    try:
        out = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        _check(be, items, masks, slots, mans, Qs, out, "masks")
        # the quantiles and the mean do not depend on the mask; the densities do
        full = be.run_credible(slots, mans, [cc.full_mask(m) for m in mans], cc.MASS, cc.PROBS, Qs)
        assert out[0]["quant"].tobytes() == full[0]["quant"].tobytes() and out[0]["mean"].tobytes() == full[0]["mean"].tobytes()
        for i, (m, k) in enumerate(zip(mans, masks)):
            assert (out[1][i].tobytes() == full[1][i].tobytes()) == (k == cc.full_mask(m)), (i, m, k)
    finally:
        be.close()


def test_batch_of_300_is_deterministic_and_equals_single_launches(hip_backend):
    """more workgroups than the chip has CUs; manifolds, clouds, counts, masks and numbers of queries (0 among them) mixed"""
    be, items, masks, slots, mans, Qs = _scenario(hip_backend, "batch")
    try:
        assert any(len(Q) == 0 for Q in Qs) and any(len(Q) > 1 for Q in Qs)
        a = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        b = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        _check(be, items, masks, slots, mans, Qs, a, "batch")
        recs, ld, od, qrecs, first = a
        for i in range(len(items)):
            r1, l1, o1, q1, f1 = be.run_credible([slots[i]], [mans[i]], [masks[i]], cc.MASS, cc.PROBS, [Qs[i]])
            assert r1[0].tobytes() == recs[i].tobytes() and l1[0].tobytes() == ld[i].tobytes() and o1[0].tobytes() == od[i].tobytes(), (i, items[i])
            assert q1.tobytes() == qrecs[first[i]:first[i + 1]].tobytes() and f1.tolist() == [0, len(Qs[i])], (i, items[i])
    finally:
        be.close()


def test_600_queries_of_one_belief_in_a_small_context(hip_backend):
    """more queries than the workgroup has lanes (64 at N = 64: ten rounds), next to beliefs with none and with one"""
    N = 64
    items = [(abi.EUCLID2, "gaussian", N), (abi.SE2, "two_cluster", N), (abi.CIRCULAR, "across_pi", 63), (abi.EUCLID3, "gaussian", N)]
    masks = [3, 7, 1, 5]
    be = hip_backend(N, len(items))
    try:
        slots, mans, Qs = _load(be, items, [0, 600, 1, 0], cc.MANY_SEED)
        assert [len(Q) for Q in Qs] == [0, 600, 1, 0]
        out = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        # (600 random queries among 64 values: a query may fall within the bound of an l_i, where numpy's count may differ by one --
        # the counts are held to the device's own values, the densities to the restatement)
        recs, ld, od, qrecs, first = out
        assert first.tolist() == [0, 0, 600, 601, 601]
        back = be.beliefs_read(slots, mans)
        for i, m in enumerate(mans):
            D, c = abi.MANIFOLD_DIM[m], len(back[i][0])
            ref = cr.credible_numpy(m, back[i][0], back[i][1], masks[i], cc.MASS, cc.PROBS, Qs[i][:, :D], mean=recs["mean"][i, :D])
            q = qrecs[first[i]:first[i + 1]]
            assert np.all(np.abs(q["logdens"] - ref.q_logdens) <= cc.l_bound(ref.q_logdens)), i
            assert np.array_equal(q["n_above"], [(ld[i, :c] > v).sum() for v in q["logdens"]]), i
            assert (q["n_above"] / c).tobytes() == q["mass"].tobytes(), i
            assert np.abs(q["n_above"] - ref.q_n_above).max(initial=0) <= 1, i
        one = be.run_credible([slots[1]], [mans[1]], [masks[1]], cc.MASS, cc.PROBS, [Qs[1][77:78]])
        assert one[3].tobytes() == qrecs[77:78].tobytes()  # a query's record depends on its belief and itself alone
    finally:
        be.close()


def test_far_query_and_own_point(hip_backend):
    """a query 1e3 bandwidths away: every term underflows, l_q is finite, n_above = c and mass = 1.0 exactly"""
    N = 200
    items = [(m, "gaussian", c) for m in (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3) for c in (N, 150)]
    be = hip_backend(N, len(items))
    try:
        slots, mans, Qs = _load(be, items, [2] * len(items), 57)
        recs, _, _, qrecs, first = be.run_credible(slots, mans, [cc.full_mask(m) for m in mans], (0.9,), (), Qs)
        for i, (m, _, c) in enumerate(items):
            own, far = qrecs[first[i]], qrecs[first[i] + 1]
            assert np.isfinite(far["logdens"]) and far["logdens"] < -4e5 * abi.MANIFOLD_DIM[m], (i, far)
            assert far["n_above"] == c and far["mass"].tobytes() == np.float64(1.0).tobytes(), (i, far)
            assert 0 <= own["n_above"] < c and own["logdens"] > recs["log_min"][i], (i, own)
    finally:
        be.close()


def test_kde_form_equals_resident_form(hip_backend):
    N = 200
    items = [(m, kind, c) for m in cc.MANIFOLDS for kind, c in (("gaussian", N), ("two_cluster", 150), ("across_pi", 63), ("gaussian", 1))]
    be = hip_backend(N, len(items) + 1)
    try:
        slots, mans, Qs = _load(be, items, [3] * len(items), 67, first_slot=1)  # slot 0 is the staging slot
        masks = [(1 + i) % (1 << abi.MANIFOLD_DIM[m]) or 1 for i, m in enumerate(mans)]
        recs, ld, od, qrecs, first = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        bel = cc.beliefs(items, [3] * len(items), 67)
        for i, (m, (X, h, Q)) in enumerate(zip(mans, bel)):
            c = len(X)
            r1, l1, o1, q1 = be.kde_credible(m, pc.to_points(m, X), h, masks[i], cc.MASS, cc.PROBS, Q)
            assert r1.tobytes() == recs[i].tobytes(), (i, items[i])
            assert l1.shape == (c,) and l1.tobytes() == ld[i, :c].tobytes() and o1.tobytes() == od[i, :c].tobytes(), (i, items[i])
            assert q1.tobytes() == qrecs[first[i]:first[i + 1]].tobytes(), (i, items[i])
            r2, l2, o2, q2 = be.kde_credible(m, pc.to_points(m, X), h, masks[i], cc.MASS, cc.PROBS, None, logdens=False, order=False)
            assert r2.tobytes() == recs[i].tobytes() and l2 is None and o2 is None and q2 is None
    finally:
        be.close()


def test_nullable_outputs_given_and_not_given(hip_backend):
    be, items, masks, slots, mans, Qs = _scenario(hip_backend, "masks")
    try:
        full = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        for logdens, order, queries in ((False, False, None), (True, False, None), (False, True, Qs), (False, False, Qs)):
            got = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, queries, logdens=logdens, order=order)
            assert got[0].tobytes() == full[0].tobytes()
            assert (got[1] is None) == (not logdens) and (got[2] is None) == (not order) and (got[3] is None) == (queries is None)
            assert got[1] is None or got[1].tobytes() == full[1].tobytes()
            assert got[2] is None or got[2].tobytes() == full[2].tobytes()
            assert got[3] is None or got[3].tobytes() == full[3].tobytes()
        none = be.run_credible(slots, mans, masks, (), ())  # no mass, no probability: counts, means and the per-particle rows
        assert np.all(none[0]["log_level"] == 0) and np.all(none[0]["quant"] == 0) and np.all(none[0]["n_inside"] == 0)
        assert none[0]["mean"].tobytes() == full[0]["mean"].tobytes() and none[1].tobytes() == full[1].tobytes()
        assert none[0]["log_min"].tobytes() == full[0]["log_min"].tobytes() and none[2].tobytes() == full[2].tobytes()
    finally:
        be.close()


def test_bad_bandwidth_gives_nan_and_keeps_the_quantiles(hip_backend):
    """zero, NaN, inf or negative in each coordinate in turn: inside the mask levels, l and query results are NaN and order is -1;
    outside the mask nothing changes; the quantiles and the mean stand either way"""
    N = 65
    cases = [(m, k, d, bad) for m in cc.MANIFOLDS for k in range(1, 1 << abi.MANIFOLD_DIM[m]) for d in range(abi.MANIFOLD_DIM[m])
             for bad in (0.0, np.nan, np.inf, -1.0)]
    items = [(m, "gaussian", (N, 63)[i % 2]) for i, (m, _, _, _) in enumerate(cases)]
    masks = [k for _, k, _, _ in cases]
    be = hip_backend(N, len(items))
    try:
        slots, mans, Qs = _load(be, items, [2] * len(items), 77)
        good = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        assert np.isfinite(good[0]["log_level"][:, :len(cc.MASS)]).all()
        back = be.beliefs_read(slots, mans)
        spoiled = []
        for (m, k, d, bad), (pts, bw, _) in zip(cases, back):
            bw = np.array(bw, dtype=np.float64)
            bw[d] = bad
            spoiled.append((pts, bw, None))
        be.beliefs_write(slots, mans, spoiled)
        recs, ld, od, qrecs, first = be.run_credible(slots, mans, masks, cc.MASS, cc.PROBS, Qs)
        back = be.beliefs_read(slots, mans)  # (the SE(2) headings have been rewritten through atan2: an ulp of theta)
        for i, (m, k, d, bad) in enumerate(cases):
            c = items[i][2]
            if k >> d & 1:
                cc.check_belief(m, k, back[i][0], back[i][1], cc.MASS, cc.PROBS, recs[i], ld[i], od[i], Qs[i], qrecs[first[i]:first[i + 1]],
                                f"spoiled {cases[i]}")
                assert np.isnan(ld[i, :c]).all() and np.all(od[i] == -1) and np.isnan(qrecs["mass"][first[i]:first[i + 1]]).all(), cases[i]
            elif m != abi.SE2:
                assert recs[i].tobytes() == good[0][i].tobytes() and ld[i].tobytes() == good[1][i].tobytes(), cases[i]
                assert qrecs[first[i]:first[i + 1]].tobytes() == good[3][first[i]:first[i + 1]].tobytes(), cases[i]
            else:
                assert np.isfinite(ld[i, :c]).all() and np.abs(ld[i, :c] - good[1][i, :c]).max() <= 1e-12 * (1 + np.abs(ld[i, :c]).max()), cases[i]
    finally:
        be.close()


def test_refusals(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    try:
        rng = np.random.default_rng(87)
        for s in (0, 1):
            be.slot_write(s, abi.EUCLID2, pc.cloud("gaussian", abi.EUCLID2, 64, rng), [0.3, 0.3])
        E2 = abi.EUCLID2
        ok = be.run_credible([0, 1], [E2, E2], [3, 1], (0.5,), (0.5,), [np.zeros((1, 2)), np.zeros((0, 2))])
        assert np.isfinite(ok[0]["log_level"][:, 0]).all()

        def refused(code, match, *a, **kw):
            with pytest.raises(iif.NbpError, match=match) as e:
                be.run_credible(*a, **kw)
            assert f"status {code}:" in str(e.value), e.value
        for bad in (-1, 4):
            refused(-4, "belief 1: slot out of range", [0, bad], [E2, E2], [3, 3])
        for bad in (0, 6):
            refused(-1, "belief 1: unknown manifold", [0, 1], [E2, bad], [3, 3])
        refused(-4, "belief 1: empty mask", [0, 1], [E2, E2], [3, 0])
        refused(-4, "belief 0: coordinate outside the manifold", [0, 1], [E2, E2], [4, 3])
        refused(-4, "belief 1: coordinate outside the manifold", [0, 1], [E2, E2], [3, -1])
        refused(-4, "n_mass outside 0 .. 8", [0], [E2], [3], (0.5,) * 9)
        refused(-4, "n_prob outside 0 .. 8", [0], [E2], [3], (), (0.5,) * 9)
        for bad in (0.0, -0.1, 1.0000001, np.nan, np.inf):
            refused(-4, r"mass 1 outside \(0, 1\]", [0], [E2], [3], (0.5, bad))
        for bad in (-1e-9, 1.0000001, np.nan, -np.inf):
            refused(-4, r"probability 2 outside \[0, 1\]", [0], [E2], [3], (), (0.0, 1.0, bad))
        for bad in (np.nan, np.inf, -np.inf):
            refused(-4, "belief 1: a query entry is not finite", [0, 1], [E2, E2], [3, 3], (), (), [np.zeros((2, 2)), np.array([[0.0, 1.0], [0.0, bad]])])
            be.run_credible([0, 1], [E2, E2], [3, 1], (), (), [np.zeros((2, 2)), np.array([[0.0, bad]])])  # outside the mask: not read
        # the raw entry point: null pointers, n = 0, a q_first that does not ascend from 0
        one, man, msk = (C.c_int32 * 1)(0), (C.c_int32 * 1)(E2), (C.c_int32 * 1)(3)
        opts = be._credible_opts((0.5,), (0.5,))
        rec, qrec = (abi.CredibleRec * 1)(), (abi.CredibilityRec * 2)()
        q = (C.c_double * 6)()
        call = lib.nbp_run_credible
        assert call(ctx, one, man, msk, 1, C.byref(opts), None, None, rec, None, None, None) == 0 and rec[0].count == 64
        assert call(ctx, None, man, msk, 1, C.byref(opts), None, None, rec, None, None, None) == -1
        assert call(ctx, one, None, msk, 1, C.byref(opts), None, None, rec, None, None, None) == -1
        assert call(ctx, one, man, None, 1, C.byref(opts), None, None, rec, None, None, None) == -1
        assert call(ctx, one, man, msk, 1, None, None, None, rec, None, None, None) == -1
        assert call(ctx, one, man, msk, 1, C.byref(opts), None, None, None, None, None, None) == -1
        assert call(None, one, man, msk, 1, C.byref(opts), None, None, rec, None, None, None) == -1
        assert call(ctx, None, None, None, 0, None, None, None, None, None, None, None) == 0  # n = 0 is NBP_OK
        for qf, want in (((0, 2), 0), ((1, 2), -4), ((0, -1), -4)):
            assert call(ctx, one, man, msk, 1, C.byref(opts), (C.c_int32 * 2)(*qf), q, rec, None, None, qrec) == want, qf
        assert b"q_first must ascend from 0" in lib.nbp_last_error()
        assert call(ctx, one, man, msk, 1, C.byref(opts), (C.c_int32 * 2)(0, 2), None, rec, None, None, qrec) == -1
        assert call(ctx, one, man, msk, 1, C.byref(opts), (C.c_int32 * 2)(0, 2), q, rec, None, None, None) == -1
        assert call(ctx, one, man, msk, 1, C.byref(opts), (C.c_int32 * 2)(0, 0), None, rec, None, None, None) == 0  # no query: not read
        pts = np.ascontiguousarray(pc.cloud("gaussian", E2, 64, rng))
        bw = np.array([0.3, 0.3])
        P, H = pts.ctypes.data_as(dp), bw.ctypes.data_as(dp)
        kde = lib.nbp_kde_credible
        assert kde(ctx, E2, P, 64, H, 3, C.byref(opts), q, 2, rec, None, None, qrec) == 0
        assert kde(ctx, E2, None, 64, H, 3, C.byref(opts), q, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 64, None, 3, C.byref(opts), q, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 64, H, 3, None, q, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 64, H, 3, C.byref(opts), None, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 64, H, 3, C.byref(opts), q, 2, None, None, None, qrec) == -1
        assert kde(ctx, 9, P, 64, H, 3, C.byref(opts), q, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 0, H, 3, C.byref(opts), q, 2, rec, None, None, qrec) == -1
        assert kde(ctx, E2, P, 64, H, 0, C.byref(opts), q, 2, rec, None, None, qrec) == -4
        assert kde(ctx, E2, P, 64, H, 4, C.byref(opts), q, 2, rec, None, None, qrec) == -4
        assert kde(ctx, E2, P, 64, H, 3, C.byref(opts), None, 0, rec, None, None, None) == 0
        # a refusal touches nothing: the context stays usable and slot 1 is what it was
        again = be.run_credible([0, 1], [E2, E2], [3, 1], (0.5,), (0.5,), [np.zeros((1, 2)), np.zeros((0, 2))])
        assert again[0][1].tobytes() == ok[0][1].tobytes() and again[1][1].tobytes() == ok[1][1].tobytes()
    finally:
        be.close()


def test_every_refusal_of_the_kde_form_comes_before_slot_0_is_touched(hip_backend):
    be = hip_backend(64, 2)
    try:
        E2, rng = abi.EUCLID2, np.random.default_rng(88)
        kept = [(np.ascontiguousarray(pc.cloud("gaussian", E2, 64, rng)), np.array([0.3, 0.2 + 0.1 * s])) for s in (0, 1)]
        for s, (p, h) in enumerate(kept):
            be.belief_write(s, E2, p, h)
        before = [be.belief_read(s, E2) for s in (0, 1)]
        other, bw, q = np.ones((64, 2)), [0.5, 0.5], np.zeros((2, 2))

        def refused(code, text, mask, mass=(0.5,), queries=None):
            with pytest.raises(iif.NbpError) as e:
                be.kde_credible(E2, other, bw, mask, mass, (0.5,), queries)
            assert str(e.value) == f"libnbp status {code}: {text}", e.value
        refused(-4, "credible: belief 0: empty mask", 0)
        refused(-4, "credible: belief 0: coordinate outside the manifold", 4)
        refused(-4, "credible: belief 0: coordinate outside the manifold", -1)
        for bad in (np.nan, np.inf):
            refused(-4, "credible: belief 0: a query entry is not finite", 2, queries=np.array([[0.0, 0.0], [0.0, bad]]))
        refused(-4, "credible: n_mass outside 0 .. 8", 3, mass=(0.5,) * 9)
        refused(-4, "credible: mass 0 outside (0, 1]", 3, mass=(0.0,))
        for s, (p, h) in enumerate(kept):
            after = be.belief_read(s, E2)
            assert after[0].tobytes() == p.tobytes() and after[1].tobytes() == h.tobytes(), s
            assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before[s])), s
        assert be.kde_credible(E2, other, bw, 1, (0.5,), (0.5,), np.array([[0.0, np.nan]]))[0]["count"] == 64  # outside the mask: not read
    finally:
        be.close()


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
def _chain(graph):
    fg = iif.initfg(iif.SolverParams(N=100))
    n = 6
    if graph == "euclid_chain6":
        for i in range(n):
            iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
        iif.addFactor(fg, ["x0"], iif.Prior(iif.Normal(0.0, 0.1)))
        for i in range(n - 1):
            iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    else:  # the graph of test/testCircular.jl:7-29, one pose longer
        for i in range(n):
            iif.addVariable(fg, f"x{i}", iif.Circular)
        iif.addFactor(fg, ["x0"], iif.PriorCircular(iif.Normal(0.0, 0.1)))
        for i in range(n - 1):
            iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.CircularCircular(iif.Normal(1.0, 0.1)))
    return fg, n


def _same_region(a, b):
    return all(np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes()
               for f in ("mass", "log_levels", "levels", "n_inside", "probs", "quantiles", "mean", "logdens", "order")) and a.count == b.count


@pytest.mark.parametrize("graph", ["euclid_chain6", "circular_chain6"])
def test_session_equals_mirror_and_moves_no_belief(hip_backend, graph):
    fg, n = _chain(graph)
    truth = {f"x{i}": [float(pc.wrap(i)) if graph == "circular_chain6" else float(i)] for i in range(n)}
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=61)
        before = dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"])
        regions, cred = ses.credibleRegions(), ses.credibility(truth)
        assert dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"]) == before
        assert list(regions) == fg.ls() == list(cred)
        host_r, host_c = iif.credibleRegionAll(fg, backend=iif.HipBackend), iif.credibility(fg, truth, backend=iif.HipBackend)
        for v in fg.ls():
            var = fg.getVariable(v)
            assert _same_region(regions[v], host_r[v]), v
            assert _same_region(regions[v], iif.credibleRegion(fg, v, backend=iif.HipBackend)), v
            assert _same_region(regions[v], iif.getBelief(fg, v).credible(backend=iif.HipBackend)), v
            for f in ("mass", "logdens", "n_above"):
                assert np.asarray(getattr(cred[v], f)).tobytes() == np.asarray(getattr(host_c[v], f)).tobytes(), (v, f)
            one = iif.getBelief(fg, v).credibility(truth[v], backend=iif.HipBackend)
            assert (one.mass, one.logdens, one.n_above) == (cred[v].mass, cred[v].logdens, cred[v].n_above), v
            reg = regions[v]
            assert reg.count == 100 and reg.quantiles.shape == (1, 5) and reg.logdens.shape == (100,) and sorted(reg.order) == list(range(100))
            for a, k in zip(reg.mass, reg.n_inside):
                assert reg.inside(a).sum() == k >= np.ceil(a * 100)
            assert np.all(np.diff(reg.log_levels) <= 0) and np.allclose(reg.levels, np.exp(reg.log_levels))
            assert 0.0 <= cred[v].mass <= 1.0 and isinstance(cred[v].n_above, int)
            # against the restatement on the host copy
            ref = cr.credible_numpy(var.varType.manifold, var.val, var.bw, 1, reg.mass, reg.probs, [truth[v]], mean=reg.mean)
            assert np.all(np.abs(reg.logdens - ref.logdens) <= cc.l_bound(ref.logdens)), v
            assert abs(cred[v].logdens - ref.q_logdens[0]) <= cc.l_bound(ref.q_logdens[0]), v
            assert reg.quantiles.tobytes() == ref.quantiles.tobytes(), v
        two = ses.credibleRegions(["x3"], mass=(0.9,), probs=(0.5,))
        assert list(two) == ["x3"] and two["x3"].log_levels[0] == regions["x3"].log_levels[1]
        assert dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"]) == before
        print(graph, "masses of the truth", {v: cred[v].mass for v in cred}, "coverage", iif.coverage(cred))
        with pytest.raises(ValueError, match="never part of a solve"):
            ses.credibleRegions(["nope"])
