"""-m gpu: the modes of beliefs on the device (nbp_run_modes / nbp_kde_modes, csrc/nbp_modes.h) through the C ABI and through the
mirror, held to the table and the criteria of tests/modes_cases.py: the number of modes each cloud must have, and the numpy
restatement's labels, counts, leaders (equal), iteration counts (+-1) and locations (tol + 1e-12, in units of the bandwidth
searched at) on the slot as read back.  Every bandwidth is set by hand."""
import copy
import ctypes as C

import numpy as np
import pytest

import modes_cases as mc
import ppe_cases as pc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
modes = iif.modes


def _load(be, items, seed):
    """items = [(manifold, cloud kind, count)] -> slot i holds belief i; returns (slots, manifolds, [(bw, scale, heavy)])"""
    rng = np.random.default_rng(seed)
    slots, mans, made = list(range(len(items))), [m for m, _, _ in items], [mc.make(kind, m, c, rng) for m, kind, c in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), bw, None) for m, (X, bw, _, _) in zip(mans, made)])
    return slots, mans, [(bw, scale, heavy) for _, bw, scale, heavy in made]


def _run(be, slots, mans, scales, **kw):
    """run_modes of all beliefs, one launch per scale -> [BeliefModes]"""
    out = [None] * len(slots)
    for s in sorted(set(scales)):
        ix = [i for i, q in enumerate(scales) if q == s]
        res = be.run_modes([slots[i] for i in ix], [mans[i] for i in ix], bw_scale=s, **kw)
        for k, i in enumerate(ix):
            out[i] = modes.modes_from_records(mans[i], *(r[k] for r in res))
    return out


def _check_all(be, items, slots, mans, made, table):
    got = _run(be, slots, mans, [scale for _, scale, _ in made])
    back = be.beliefs_read(slots, mans)
    _, point, _ = be.run_ppe(slots, mans)  # `max` of an all-identical belief: point 0 as the slot holds it
    for i, (m, kind, c) in enumerate(items):
        pts, bw, _ = back[i]
        (bw0, scale, heavy), D = made[i], abi.MANIFOLD_DIM[m]
        assert len(pts) == c and np.array_equal(bw, bw0)
        X = coords(m, pts)
        what = f"[{i}] manifold {m} {kind} c={c} N={be.N}"
        assert len(got[i].labels) == c and len(got[i].iters) == c
        if table or kind == "identical" or c == 1:
            mc.check_table("identical" if c == 1 else kind, m, X, got[i], heavy, what, point[i, :D])
        mc.check_device(m, X, bw, scale, got[i], modes.modes_numpy(m, pts, bw, scale), what=what)


@pytest.mark.parametrize("N", mc.SIZES)
def test_every_manifold_and_cloud_at_full_count(hip_backend, N):
    items = [(m, kind, N) for m in mc.MANIFOLDS for kind in mc.TABLE_CLOUDS + (("doors4",) if m in (abi.CIRCULAR, abi.SE2) else ())]
    be = hip_backend(N, len(items))
    try:
        slots, mans, made = _load(be, items, 400 + N)
        _check_all(be, items, slots, mans, made, table=True)
    finally:
        be.close()


def test_counts_below_the_context_size(hip_backend):
    items = [(m, kind, c) for m in mc.MANIFOLDS for c in (1, 2, 63, 150) for kind in ("gaussian", "two_cluster", "across_pi")]
    be = hip_backend(200, len(items))
    try:
        slots, mans, made = _load(be, items, 7)
        _check_all(be, items, slots, mans, made, table=False)
        res = be.run_modes(slots, mans)
        for i, (m, kind, c) in enumerate(items):  # the rows beyond the count
            assert np.all(res[2][i, c:] == -1) and np.all(res[3][i, c:] == 0) and np.all(res[2][i, :c] >= 0) and np.all(res[3][i, :c] >= 1)
    finally:
        be.close()


def _batch_items(n, N, seed):
    rng = np.random.default_rng(seed)
    kinds = mc.TABLE_CLOUDS + ("doors4",)
    return [(mc.MANIFOLDS[rng.integers(5)], kinds[rng.integers(5)], int(rng.choice([N, N, N, 150, 63, 2, 1]))) for _ in range(n)]


def test_batch_of_300_mixed_beliefs_is_deterministic_and_equals_single_calls(hip_backend):
    """more workgroups than the chip has CUs, manifolds, counts and numbers of iterations mixed in one launch"""
    items = _batch_items(300, 200, 21)
    be = hip_backend(200, len(items))
    try:
        slots, mans, made = _load(be, items, 22)
        a = be.run_modes(slots, mans)
        b = be.run_modes(slots, mans)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for i in range(len(items)):
            one = be.run_modes([slots[i]], [mans[i]])
            for x, y in zip(a, one):
                assert x[i].tobytes() == y[0].tobytes(), (i, items[i])
        back = be.beliefs_read(slots[:24], mans[:24])
        for i in range(24):
            m, (pts, bw, _) = mans[i], back[i]
            mc.check_device(m, coords(m, pts), bw, 2.0, modes.modes_from_records(m, *(r[i] for r in a)), modes.modes_numpy(m, pts, bw),
                            what=f"[{i}] {items[i]}")
    finally:
        be.close()


def test_bad_bandwidth_gives_no_modes(hip_backend):
    """one entry of the bandwidth zero, NaN, infinite or negative (each coordinate of the manifold takes its turn)"""
    N = 200
    items = [(m, "gaussian", c) for m in mc.MANIFOLDS for c in (N, 63)]
    be = hip_backend(N, len(items))
    rng = np.random.default_rng(31)
    try:
        slots, mans = list(range(len(items))), [m for m, _, _ in items]
        for k, bad in enumerate((0.0, np.nan, np.inf, -1.0, 0.0, np.nan)):
            bws = []
            for m in mans:
                bw = pc.hand_bandwidth(m).copy()
                bw[k % len(bw)] = bad
                bws.append(bw)
            be.beliefs_write(slots, mans, [(pc.to_points(m, pc.cloud(kind, m, c, rng)), bws[i], None) for i, (m, kind, c) in enumerate(items)])
            recs, nm, lab, its, unc = be.run_modes(slots, mans)
            assert np.all(nm == 0) and np.all(lab == -1) and np.all(its == 0) and np.all(unc == 0), (k, nm)
            for i, m in enumerate(mans):
                D = abi.MANIFOLD_DIM[m]
                assert np.isnan(recs["location"][i, :, :D]).all() and np.all(recs["location"][i, :, D:] == 0), (k, i)
                assert np.isnan(recs["density"][i]).all() and np.all(recs["count"][i] == 0) and np.all(recs["leader"][i] == -1)
                bm = modes.modes_from_records(m, *(r[i] for r in (recs, nm, lab, its, unc)))
                assert bm.n_modes == 0 and bm.modes.shape == (0, D)
        # a scale that takes a good bandwidth out of the finite numbers is the same refusal
        be.beliefs_write(slots, mans, [(pc.to_points(m, pc.cloud(kind, m, c, rng)), pc.hand_bandwidth(m) * 1e300, None) for m, kind, c in items])
        recs, nm, lab, its, unc = be.run_modes(slots, mans, bw_scale=1e10)
        assert np.all(nm == 0) and np.all(lab == -1)
    finally:
        be.close()


def test_host_buffer_form_equals_the_resident_form(hip_backend):
    N = 200
    items = [(m, kind, c) for m in mc.MANIFOLDS for kind, c in (("gaussian", N), ("two_cluster", N), ("across_pi", 150), ("gaussian", 1))]
    be = hip_backend(N, len(items) + 1)
    try:
        rng = np.random.default_rng(41)
        slots, mans = list(range(1, len(items) + 1)), [m for m, _, _ in items]  # slot 0 is the staging slot of nbp_kde_modes
        made = [mc.make(kind, m, c, rng) for m, kind, c in items]
        pts = [pc.to_points(m, X) for m, (X, _, _, _) in zip(mans, made)]
        be.beliefs_write(slots, mans, [(p, bw, None) for p, (_, bw, _, _) in zip(pts, made)])
        recs, nm, lab, its, unc = be.run_modes(slots, mans, bw_scale=1.5)
        for i, (m, kind, c) in enumerate(items):
            r1, n1, l1, i1, u1 = be.kde_modes(m, pts[i], made[i][1], bw_scale=1.5)
            assert r1.tobytes() == recs[i].tobytes() and n1 == nm[i] and u1 == unc[i], (i, items[i])
            assert np.array_equal(l1, lab[i, :c]) and np.array_equal(i1, its[i, :c]) and len(l1) == c, (i, items[i])
            bm = iif.Belief(m, pts[i], made[i][1]).modes(bwScale=1.5, backend=be)  # the mirror takes the same road
            assert bm.modes.tobytes() == recs["location"][i, :nm[i], :abi.MANIFOLD_DIM[m]].tobytes() and np.array_equal(bm.labels, l1)
    finally:
        be.close()


def test_max_iter_is_reported(hip_backend):
    N = 200
    items = [(m, "two_cluster", c) for m in mc.MANIFOLDS for c in (N, 150)]
    be = hip_backend(N, len(items))
    try:
        slots, mans, made = _load(be, items, 51)
        recs, nm, lab, its, unc = be.run_modes(slots, mans, bw_scale=1.0, max_iter=3)
        full = be.run_modes(slots, mans, bw_scale=1.0)
        for i, (m, kind, c) in enumerate(items):
            assert unc[i] > 0 and its[i, :c].max() == 3 and its[i, :c].min() >= 1 and np.all(its[i, c:] == 0), (i, unc[i], its[i])
            assert unc[i] == int((full[3][i, :c] > 3).sum()), (i, unc[i])  # the starts that take more than three iterations
            assert np.array_equal(its[i, :c], np.minimum(full[3][i, :c], 3))
            assert full[4][i] == 0 and nm[i] >= full[1][i] == 2
    finally:
        be.close()


def test_argument_errors_behave_as_run_ppes_do(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp = C.POINTER(C.c_double)
    try:
        rng = np.random.default_rng(61)
        be.slot_write(0, abi.EUCLID2, pc.cloud("gaussian", abi.EUCLID2, 64, rng), [0.3, 0.4])
        for bad in (-1, 4):
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_modes([bad], [abi.EUCLID2])
        for bad in (0, 6):
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_modes([0], [bad])
        for kw in (dict(bw_scale=0.0), dict(bw_scale=np.inf), dict(bw_scale=np.nan), dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0),
                   dict(merge=0.0), dict(merge=np.inf)):
            with pytest.raises(iif.NbpError, match="-1"):
                be.run_modes([0], [abi.EUCLID2], **kw)
        for kw in (dict(tol=1e-4), dict(merge=9.99e-4)):
            with pytest.raises(iif.NbpError, match="-4"):
                be.run_modes([0], [abi.EUCLID2], **kw)
        one, man, nm = (C.c_int32 * 1)(0), (C.c_int32 * 1)(abi.EUCLID2), (C.c_int32 * 1)()
        recs = (abi.ModeRec * abi.MODES_MAX)()
        assert lib.nbp_run_modes(ctx, None, man, 1, None, recs, nm, None, None, None) == -1
        assert lib.nbp_run_modes(ctx, one, None, 1, None, recs, nm, None, None, None) == -1
        assert lib.nbp_run_modes(ctx, one, man, 1, None, None, nm, None, None, None) == -1
        assert lib.nbp_run_modes(ctx, one, man, 1, None, recs, None, None, None, None) == -1
        assert lib.nbp_run_modes(None, one, man, 1, None, recs, nm, None, None, None) == -1
        assert lib.nbp_run_modes(ctx, None, None, 0, None, None, None, None, None, None) == 0  # n = 0 is NBP_OK
        assert lib.nbp_run_modes(ctx, one, man, 1, None, recs, nm, None, None, None) == 0       # options and the per-point outputs are optional
        assert nm[0] == 1 and recs[0].count == 64 and recs[1].leader == -1
        pts = np.ascontiguousarray(pc.cloud("gaussian", abi.EUCLID2, 64, rng))
        bw = np.array([0.3, 0.4])
        assert lib.nbp_kde_modes(ctx, abi.EUCLID2, None, 64, bw.ctypes.data_as(dp), None, recs, nm, None, None, None) == -1
        assert lib.nbp_kde_modes(ctx, abi.EUCLID2, pts.ctypes.data_as(dp), 64, None, None, recs, nm, None, None, None) == -1
        assert lib.nbp_kde_modes(ctx, 9, pts.ctypes.data_as(dp), 64, bw.ctypes.data_as(dp), None, recs, nm, None, None, None) == -1
        assert lib.nbp_kde_modes(ctx, abi.EUCLID2, pts.ctypes.data_as(dp), 0, bw.ctypes.data_as(dp), None, recs, nm, None, None, None) == -1
        opts = abi.ModesOpts(bw_scale=2.0, tol=1e-6, merge=1e-4, max_iter=10)
        assert lib.nbp_kde_modes(ctx, abi.EUCLID2, pts.ctypes.data_as(dp), 64, bw.ctypes.data_as(dp), C.byref(opts), recs, nm, None, None, None) == -4
        assert lib.nbp_kde_modes(ctx, abi.EUCLID2, pts.ctypes.data_as(dp), 64, bw.ctypes.data_as(dp), None, recs, nm, None, None, None) == 0
        # the context stays usable
        res = be.run_modes([0], [abi.EUCLID2])
        assert res[1][0] == 1 and res[4][0] == 0 and np.isfinite(res[0]["location"][0, 0]).all()
    finally:
        be.close()


def test_session_reports_the_modes_of_resident_beliefs_without_moving_them(hip_backend):
    """the circular-doors canonical graph (multihypo sightings of four doors): after a solve, the modes of every belief from ONE launch
    on the resident beliefs; `stats` does not move, and every answer is the restatement's on the host copy of the belief"""
    fg = iif.generateCircularDoors(nposes=20, N=200, sightEvery=5)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=71)
        before = copy.deepcopy(ses.stats)
        got = ses.getBeliefModes()
        assert ses.stats == before
        assert list(got) == list(ses._labels) and len(got) == 24
        for v, bm in got.items():
            var = fg.getVariable(v)
            m = var.varType.manifold
            ref = iif.modes_numpy(m, var.val, var.bw)
            print(f"{v}: {bm.n_modes} modes, shares {np.round(bm.shares, 3).tolist()}, at {np.round(bm.modes[:, 0], 3).tolist()}")
            mc.check_device(m, coords(m, var.val), var.bw, 2.0, bm, ref, what=v)
        one = ses.getBeliefModes(["x7"], bwScale=1.0)
        assert list(one) == ["x7"] and ses.stats == before
        var = fg.getVariable("x7")
        mc.check_device(abi.CIRCULAR, coords(abi.CIRCULAR, var.val), var.bw, 1.0, one["x7"], iif.modes_numpy(abi.CIRCULAR, var.val, var.bw, 1.0), what="x7 at scale 1")
        assert got["l0"].n_modes == 1 and abs(pc.wrap(got["l0"].modes[0, 0] + 2.4)) < 0.05  # a door stands where its prior puts it
        with pytest.raises(ValueError):
            ses.getBeliefModes(merge=1e-5)
