"""-m gpu: scene densities on the device (nbp_run_scene_grid, csrc/nbp_scene.h) through the C ABI, the mirror and the session, held to
the criteria of tests/scene_cases.py: bit-equal to the device's own marginal grids where the definition promises it (one belief; the
sum in list order without culling), within 1e-12 relative (+ the clamp's floor) of the exact sums of scene_grid_numpy at every reach,
exact zeros and no owner where no belief reaches, extents bit-equal to the numpy arithmetic, owners by the owner criterion.

Contexts hold 16 .. 80 particles and the grids at most 96 x 40 points: the shapes are those of scene_cases (counts around the chunks of
32 and 64 particles, grids around the tile, lists around the 64 records of one ballot), not the sizes of a real map."""
import copy
import ctypes as C

import numpy as np
import pytest

import scene_cases as scs
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
sc = iif.scene
E1, E2, E3, CI, SE2 = scs.E1, scs.E2, scs.E3, scs.CI, scs.SE2
INF = np.inf


def _marginal_sum(be, slots, mans, held, n, ext):
    """the device's own marginal grids on the common extent, added on the host in list order"""
    k = len(n)
    grids = be.run_marginal_grid([(s, m, b[3], n, ext[:2 * k]) for s, m, b in zip(slots, mans, held)])
    total = np.zeros(n)
    for g in grids:
        total = total + g
    return total


# ---- 7. one belief: the marginal grid, bit for bit ---------------------------------------------------------------------------------------
def test_one_belief_is_its_marginal_grid_bit_for_bit(hip_backend):
    N = 80
    specs2 = [(m, d, scs.COUNTS[i % len(scs.COUNTS)]) for i, (m, d) in enumerate(scs.DIMS_2D)]
    specs1 = [(m, d, scs.COUNTS[(i + 3) % len(scs.COUNTS)]) for i, (m, d) in enumerate(scs.DIMS_1D * len(scs.SIZES_1D))]
    scene = scs.compact(specs2 + specs1, 101)
    assert {len(b[1]) for b in scene[:len(specs2)]} == set(scs.COUNTS) and all(len(b[1]) < N for b in scene)
    be = hip_backend(N, len(scene))
    rng = np.random.default_rng(102)
    try:
        slots, mans, held = scs.write(be, scene)
        seen = set()
        for i, b in enumerate(held):
            two = len(b[3]) == 2
            n = scs.GRIDS[i % len(scs.GRIDS)] if two else (scs.SIZES_1D[(i - len(specs2)) // 2],)
            seen.add(n)
            ext = scs.explicit_extent([b], n, rng)
            want = be.run_marginal_grid([(slots[i], mans[i], b[3], n, ext)])[0]
            got, used, own, skipped, tb = be.run_scene_grid([slots[i]], [mans[i]], b[3], n, ext, reach=INF, owner=True)
            assert got.tobytes() == want.tobytes(), (i, b[0], b[3], n, len(b[1]))
            assert used[:len(ext)].tobytes() == ext.tobytes() and np.all(used[len(ext):] == 0) and not skipped.any()
            assert tb == scs.n_tiles(n) and np.all(own[got > 0] == 0) and np.all(own[got == 0] == -1)
            # the automatic extent of a scene of one belief is the marginal grid's
            if min(n) >= 2:
                wa, ea = be.run_marginal_grid([(slots[i], mans[i], b[3], n, None, 3.0)], return_extent=True)
                ga, ua, _, _, _ = be.run_scene_grid([slots[i]], [mans[i]], b[3], n, None, margin=3.0, reach=INF)
                assert ua.tobytes() == ea[0].tobytes() and ga.tobytes() == wa[0].tobytes(), (i, b[0], b[3], n)
        assert seen == set(scs.GRIDS) | {(k,) for k in scs.SIZES_1D}
    finally:
        be.close()


# ---- 8, 9, 10, 13, 15: lists of every length, at every reach -------------------------------------------------------------------------------
def _check_list(be, scene, n, seed, what):
    rng = np.random.default_rng(seed)
    slots, mans, held = scs.write(be, scene)
    V, k = len(held), len(n)
    dims = [b[3] for b in held]
    tiles = scs.n_tiles(n)
    # 13: the automatic extent, by bytes
    autos = (None,) if scs.can_auto(held, n) else ()     # (a Euclidean axis of one point has no automatic extent)
    auto = sc.scene_extent_numpy(held, n, 4.0) if autos else None
    # 8: unit weights, no culling: the device's own marginal grids added in list order
    for ext in autos + (scs.explicit_extent(held, n, rng),):
        got, used, _, skipped, tb = be.run_scene_grid(slots, mans, dims, n, ext, reach=INF)
        assert used.tobytes() == (auto if ext is None else np.r_[ext, np.zeros(4 - 2 * k)]).tobytes(), (what, used, auto)
        assert got.tobytes() == _marginal_sum(be, slots, mans, held, n, used).tobytes(), (what, "sum of marginals", ext is None)
        assert tb == tiles * V and not skipped.any()
    # 9: against the restatement at every reach, weighted; 10: exact zeros and no owner where nobody reaches; 15: twice, and both instances
    w = rng.uniform(0.25, 4.0, V)
    zeros = 0
    for reach in scs.REACHES:
        for ext in autos + (scs.explicit_extent(held, n, rng),):
            lo, step = (None, None) if ext is None else (ext[0::2], ext[1::2])
            ref, rext, rown, _ = sc.scene_grid_numpy(held, n, lo, step, reach=reach, weights=w, owner=True)
            got, used, own, skipped, tb = be.run_scene_grid(slots, mans, dims, n, ext, reach=reach, weights=w, owner=True)
            assert used.tobytes() == rext.tobytes()
            scs.check_values(held, got, ref, w, f"{what} reach {reach} {'auto' if ext is None else 'explicit'}")
            assert np.array_equal(got == 0.0, ref == 0.0) or reach == INF     # (without culling a far term underflows on the host only)
            unreached = rown < 0
            if reach != INF:
                assert np.all(got[unreached] == 0.0) and np.all(own[unreached] == -1) and np.all(own[~unreached] >= 0)
                zeros += int(unreached.sum())
            assert tb == scs.tile_hits(held, n, used, reach), (what, reach, tb)
            again = be.run_scene_grid(slots, mans, dims, n, ext, reach=reach, weights=w, owner=True)
            plain = be.run_scene_grid(slots, mans, dims, n, ext, reach=reach, weights=w)
            assert again[0].tobytes() == got.tobytes() and again[2].tobytes() == own.tobytes() and again[4] == tb
            assert plain[0].tobytes() == got.tobytes() and plain[2] is None and plain[4] == tb
    return zeros


@pytest.mark.parametrize("V", scs.LIST_V)
def test_lists_of_poses_and_landmarks(hip_backend, V):
    """SE(2) poses on (x, y) mixed with Euclid(2) landmarks, far apart against their bandwidths; N = 16, some beliefs of 9 points"""
    n = scs.GRIDS[scs.LIST_V.index(V)]
    specs = [((SE2, E2)[i % 2], (0, 1), 16 if i % 3 else 9) for i in range(V)]
    be = hip_backend(16, V)
    try:
        zeros = _check_list(be, scs.spread(specs, 110 + V), n, 111 + V, f"V={V} n={n}")
        assert zeros > 0 or min(n) == 1 or V >= 63
    finally:
        be.close()


@pytest.mark.parametrize("case", [
    ("euclid3 (0,2)", [(E3, (0, 2), c) for c in (31, 32, 33, 64, 65, 2, 1)], (33, 65), 80),
    ("euclid3 (2,1) + euclid2 (1,0)", [(E3, (2, 1), 33), (E2, (1, 0), 64), (E3, (1, 0), 20)], (96, 40), 64),
    ("se2 (x,theta)", [(SE2, (0, 2), 33)] * 5, (31, 33), 64),
    ("se2 (theta,y)", [(SE2, (2, 1), 31)] * 4 + [(SE2, (2, 1), 64)], (32, 32), 64),
    ("euclid1", [(E1, (0,), c) for c in (64, 65, 63, 1, 2, 31)], (130,), 80),
    ("euclid1 + euclid3 (z) + se2 (y)", [(E1, (0,), 16), (E3, (2,), 9), (SE2, (1,), 16)] * 22, (65,), 16),
    ("circular + se2 (theta)", [(CI, (0,), 33), (SE2, (2,), 32), (CI, (0,), 64)], (63,), 64),
    ("circular x 65", [(CI, (0,), 16)] * 65, (64,), 16),
    ("one point", [(E2, (0, 1), 5)] * 3, (1, 1), 16),
    ("one circular point", [(CI, (0,), 5)] * 2, (1,), 16),
], ids=lambda c: c[0])
def test_lists_on_other_coordinates(hip_backend, case):
    what, specs, n, N = case
    be = hip_backend(N, len(specs))
    try:
        _check_list(be, scs.spread(specs, 120), n, 121, what)
    finally:
        be.close()


# ---- 11, 12: beliefs that add nothing; doubled weights ----------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [True, False], ids=["2-D", "1-D"])
def test_beliefs_that_add_nothing_change_no_bit_and_doubled_weights_double(hip_backend, two):
    N = 64
    rng = np.random.default_rng(131)
    if two:
        base = scs.poses_and_landmarks(5, 4, 33, 132)
        n, far, dims = (33, 65), [200.0, -150.0, 0.0], (0, 1)
    else:
        base = scs.compact([(E1, (0,), 33), (E3, (1,), 40), (SE2, (0,), 64)] * 2, 133)
        n, far, dims = (130,), [200.0, 200.0, 200.0], None
    extra = []   # (position in the longer list, belief, weight): wholly outside the extent, weight 0, unusable
    for pos, kind in ((0, "far"), (3, "zero"), (4, "unusable"), (len(base) + 3, "far"), (len(base) + 4, "unusable")):
        m, X, bw, d = base[pos % len(base)]
        if kind == "far":
            b, wv = (m, X + np.asarray(far)[:X.shape[1]], bw, d), 1.5
        elif kind == "zero":
            b, wv = (m, X.copy(), bw, d), 0.0
        else:
            h = bw.copy()
            h[d[-1]] = (0.0, np.nan)[pos % 2]
            b, wv = (m, X.copy(), h, d), 2.0
        extra.append((pos, b, wv, kind))
    w = rng.uniform(0.5, 2.0, len(base))
    longer, wl, origin = list(base), list(w), list(range(len(base)))
    for pos, b, wv, kind in extra:
        longer.insert(pos, b)
        wl.insert(pos, wv)
        origin.insert(pos, -1)
    kind_at = {pos: kind for pos, _, _, kind in extra}     # (ascending positions: an extra belief ends up at its own)
    assert all(origin[pos] == -1 for pos in kind_at)
    be = hip_backend(N, len(base) + len(longer))
    try:
        s0, m0, h0 = scs.write(be, base)
        s1, m1, h1 = scs.write(be, longer, first=len(base))
        ext = scs.explicit_extent(h0, n, rng)
        for reach in (6.0, 1.5, INF):
            a = be.run_scene_grid(s0, m0, [b[3] for b in h0], n, ext, reach=reach, weights=w, owner=True)
            keep = [(i, o) for i, o in enumerate(origin) if o >= 0 or reach != INF or kind_at[i] != "far"]
            idx = [i for i, _ in keep]     # (without culling a belief far away still adds its clamped tail: it is left out of that run)
            b = be.run_scene_grid([s1[i] for i in idx], [m1[i] for i in idx], [h1[i][3] for i in idx], n, ext, reach=reach,
                                  weights=[wl[i] for i in idx], owner=True)
            assert b[0].tobytes() == a[0].tobytes(), (reach, "grid")
            back = np.array([o for _, o in keep] + [-1])     # list index of the longer run -> of the shorter one (-1 stays -1)
            assert np.all(back[b[2]][b[2] >= 0] >= 0) and np.array_equal(back[b[2]], a[2]), (reach, "owner")
            assert b[3].tolist() == [int(o < 0 and not scs.usable(longer[i])) for i, o in keep] and not a[3].any()
            # 12: every weight doubled: every value doubled, exactly, and the same owners
            d2 = be.run_scene_grid(s0, m0, [b_[3] for b_ in h0], n, ext, reach=reach, weights=2 * w, owner=True)
            assert np.array_equal(d2[0], 2 * a[0]) and d2[2].tobytes() == a[2].tobytes(), reach
        # every belief unusable: a grid of zeros, finite, nobody's; the automatic extent falls back to lo = step = 0 on Euclidean axes
        bad = [i for i, (o, bl) in enumerate(zip(origin, longer)) if o < 0 and not scs.usable(bl)]
        g, used, own, skipped, tb = be.run_scene_grid([s1[i] for i in bad], [m1[i] for i in bad], [h1[i][3] for i in bad], n, None, owner=True)
        assert not g.any() and np.all(own == -1) and skipped.all() and tb == 0 and not used.any()
    finally:
        be.close()


# ---- 14: the owner ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(scs.owner_cases()))
def test_owner_is_the_restatements(hip_backend, name):
    scene, n, reach = scs.owner_cases()[name]
    be = hip_backend(64, len(scene))
    try:
        slots, mans, held = scs.write(be, scene)
        w = np.random.default_rng(141).uniform(0.5, 2.0, len(held))
        for weights in (None, w):
            ref, ext, rown, _, stack = sc.scene_grid_numpy(held, n, reach=reach, weights=weights, owner=True, terms=True)
            got, used, own, _, _ = be.run_scene_grid(slots, mans, [b[3] for b in held], n, None, reach=reach, weights=weights, owner=True)
            assert used.tobytes() == ext.tobytes()
            scs.check_values(held, got, ref, weights, name)
            scs.check_owner(held, own, stack, ref, weights, name)
    finally:
        be.close()


# ---- 16: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_belief_and_write_nothing(hip_backend):
    be = hip_backend(16, 4)
    lib, ctx = be.lib, be._ctx
    scene = scs.compact([(E2, (0, 1), 16), (SE2, (0, 1), 16), (CI, (0,), 16), (E3, (0, 1), 9)], 151)
    RANGE, ARG = -4, -1
    try:
        slots, mans, held = scs.write(be, scene)

        def call(slots=(0, 1, 3), mans=(E2, SE2, E3), dims=((0, 1), (0, 1), (0, 1)), w=(1.0, 1.0, 1.0), n=(5, 6), flags=0, lo=(0.0, 0.0),
                 step=(0.1, 0.1), margin=4.0, reach=6.0, null=()):
            V = len(slots)
            g = abi.SceneDesc(flags=flags, margin=margin, reach=reach)
            g.n[0], g.n[1], g.lo[0], g.lo[1], g.step[0], g.step[1] = n[0], n[1], lo[0], lo[1], step[0], step[1]
            pts = 64
            out, own = np.full(pts, 7.0), np.full(pts, 7, dtype=np.int32)
            skipped, ext, tb = np.full(max(V, 1), 7, dtype=np.int32), np.full(4, 7.0), C.c_int64(7)
            ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
            a = {"slots": np.array(slots, dtype=np.int32), "mans": np.array(mans, dtype=np.int32),
                 "dims": np.array(dims, dtype=np.int32).reshape(-1), "w": None if w is None else np.array(w, dtype=np.float64)}
            p = {k: (None if (v is None or k in null) else v.ctypes.data_as(dp if v.dtype == np.float64 else ip)) for k, v in a.items()}
            rc = lib.nbp_run_scene_grid(None if "ctx" in null else ctx, p["slots"], p["mans"], p["dims"], p["w"], V,
                                        None if "desc" in null else C.byref(g), None if "out" in null else out.ctypes.data_as(dp),
                                        own.ctypes.data_as(ip), skipped.ctypes.data_as(ip), ext.ctypes.data_as(dp), C.byref(tb))
            untouched = np.all(out == 7.0) and np.all(own == 7) and np.all(skipped == 7) and np.all(ext == 7.0) and tb.value == 7
            return rc, lib.nbp_last_error().decode(), untouched

        assert call()[0] == 0 and not call()[2]
        AUTO = abi.SCENE_AUTO_EXTENT
        table = [
            # NBP_ERR_RANGE
            (RANGE, 1, dict(slots=(0, 4, 3))),                                     # a slot outside the context
            (RANGE, 2, dict(slots=(0, 1, -1))),
            (RANGE, 0, dict(dims=((0, 2), (0, 1), (0, 1)))),                       # a coordinate outside the manifold
            (RANGE, 1, dict(dims=((0, 1), (3, 1), (0, 1)))),
            (RANGE, 2, dict(dims=((0, 1), (0, 1), (-1, 1)))),
            (RANGE, 2, dict(dims=((0, 1), (0, 1), (1, 1)))),                       # a repeated coordinate
            (RANGE, None, dict(n=(0, 6))),                                         # n outside 1 .. NBP_SCENE_MAX
            (RANGE, None, dict(n=(5, abi.SCENE_MAX + 1))),
            (RANGE, None, dict(n=(4096, 2048))),                                   # n0 n1 > 2^22
            (RANGE, None, dict(n=(1, 6), flags=AUTO)),                             # n < 2 on a Euclidean axis with the automatic extent
            (RANGE, None, dict(n=(5, 1), flags=AUTO)),
            (RANGE, None, dict(lo=(np.nan, 0.0))),                                 # a non-finite lo
            (RANGE, None, dict(lo=(0.0, -np.inf))),
            (RANGE, None, dict(step=(0.0, 0.1))),                                  # a step that is not finite and positive
            (RANGE, None, dict(step=(0.1, -0.1))),
            (RANGE, None, dict(step=(np.inf, 0.1))),
            (RANGE, None, dict(step=(0.1, np.nan))),
            (RANGE, None, dict(slots=(2,), mans=(CI,), dims=((0, -1),), w=None, n=(5, 6))),   # a 1-D scene has n[1] = 1
            # NBP_ERR_ARG
            (ARG, 1, dict(mans=(E2, 9, E3))),                                      # an unknown manifold
            (ARG, 2, dict(slots=(0, 1, 1), mans=(E2, SE2, SE2), dims=((0, 1), (0, 1), (0, 2)))),   # inadmissible against belief 0: kind
            (ARG, 1, dict(dims=((0, 1), (0, -1), (0, 1)))),                        # ... and number
            (ARG, 1, dict(slots=(2, 0), mans=(CI, E2), dims=((0, -1), (0, -1)), w=None, n=(5, 1))),
            (ARG, 0, dict(w=(-1.0, 1.0, 1.0))),                                    # a weight that is negative or not finite
            (ARG, 2, dict(w=(1.0, 1.0, np.inf))),
            (ARG, 1, dict(w=(1.0, np.nan, 1.0))),
            (ARG, None, dict(margin=np.nan)), (ARG, None, dict(margin=np.inf, flags=AUTO)),
            (ARG, None, dict(reach=np.nan)), (ARG, None, dict(reach=0.0)), (ARG, None, dict(reach=-6.0)),
            (ARG, None, dict(flags=2)),
            (ARG, None, dict(null=("ctx",))), (ARG, None, dict(null=("desc",))), (ARG, None, dict(null=("out",))),
            (ARG, None, dict(null=("slots",))), (ARG, None, dict(null=("mans",))), (ARG, None, dict(null=("dims",))),
        ]
        for status, index, kw in table:
            rc, msg, untouched = call(**kw)
            assert rc == status and untouched, (kw, rc, msg)
            if index is not None:
                assert f"belief {index}:" in msg, (kw, msg)
        # what is allowed: reach = +inf, a 1 x 1 grid on circular axes with the automatic extent, V = 0 (zeros, nobody's)
        assert call(reach=np.inf)[0] == 0
        assert call(slots=(2,), mans=(CI,), dims=((0, -1),), w=None, n=(1, 1), flags=AUTO)[0] == 0
        g = abi.SceneDesc(margin=4.0, reach=6.0)
        g.n[0], g.n[1], g.step[0], g.step[1] = 3, 2, 0.5, 0.25
        out, own, ext, tb = np.full(6, 7.0), np.full(6, 7, dtype=np.int32), np.full(4, 7.0), C.c_int64(7)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        assert lib.nbp_run_scene_grid(ctx, None, None, None, None, 0, C.byref(g), out.ctypes.data_as(dp), own.ctypes.data_as(ip), None,
                                      ext.ctypes.data_as(dp), C.byref(tb)) == 0
        assert not out.any() and np.all(own == -1) and ext.tolist() == [0.0, 0.5, 0.0, 0.25] and tb.value == 0
        assert lib.nbp_run_scene_grid(ctx, None, None, None, None, -1, C.byref(g), out.ctypes.data_as(dp), None, None, None, None) == ARG
        # the mirror raises, naming the status and the belief; the context stays usable and the slots hold what they held
        with pytest.raises(iif.NbpError, match=r"-4.*belief 1:"):
            be.run_scene_grid([0, 4], [E2, E2], (0, 1), (5, 6), [0, 0.1, 0, 0.1])
        with pytest.raises(iif.NbpError, match=r"-1.*belief 1:.*admissible"):
            be.run_scene_grid([0, 2], [E2, CI], [[0, 1], [0, -1]], (5, 6), [0, 0.1, 0, 0.1])
        got = be.run_scene_grid(slots[:2], mans[:2], (0, 1), (17, 33), None, reach=INF)
        ref = sc.scene_grid_numpy(held[:2], (17, 33), reach=INF)
        assert got[1].tobytes() == ref[1].tobytes()
        scs.check_values(held[:2], got[0], ref[0], None, "after refusals")
    finally:
        be.close()


# ---- 17: the mirror and the session -----------------------------------------------------------------------------------------------------
def _pose_landmark_graph():
    fg = iif.initfg(iif.SolverParams(N=64))
    s = np.diag([0.01, 0.01, 0.0025])
    for i in range(5):
        iif.addVariable(fg, f"x{i}", iif.SpecialEuclidean2)
    iif.addFactor(fg, ["x0"], iif.ManifoldPrior(np.zeros(3), iif.MvNormal(np.zeros(3), s)))
    for i in range(4):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.ManifoldFactor(iif.MvNormal([1.0, 0.0, 0.0], s)))
    for k in range(3):
        iif.addVariable(fg, f"l{k}", iif.ContinuousEuclid(2))
        iif.addFactor(fg, [f"l{k}"], iif.Prior(iif.MvNormal([1.5 * k, 0.7], [0.1, 0.1])))
    iif.addFactor(fg, ["l0", "l1"], iif.LinearRelative(iif.MvNormal([1.5, 0.0], [0.1, 0.1])))
    return fg


@pytest.mark.parametrize("make,n_vars", [(lambda: iif.generateChainEuclid(8, vardims=2, priorEvery=4, N=64), 8), (_pose_landmark_graph, 8)],
                         ids=["euclid2 chain", "se2 poses + landmarks"])
def test_session_draws_the_resident_beliefs_without_moving_them(hip_backend, make, n_vars):
    fg = make()
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=171)
        before = copy.deepcopy(ses.stats)
        got = ses.sceneGrid(n=(96, 40), owner=True)
        sub = ses.sceneGrid("^x[12]$", n=33, reach=3.0, weights={"x2": 2.0})
        assert ses.stats == before      # no belief travelled
        want = iif.sceneGrid(fg, n=(96, 40), owner=True, backend=iif.HipBackend)
        assert got.labels == want.labels and len(got.labels) == n_vars and got.skipped == [] == want.skipped
        assert got.grid.tobytes() == want.grid.tobytes() and got.owner.tobytes() == want.owner.tobytes()
        assert got.extent.tobytes() == want.extent.tobytes() and got.tile_beliefs == want.tile_beliefs > 0
        wsub = iif.sceneGrid(fg, ["x1", "x2"], n=33, reach=3.0, weights={"x2": 2.0}, backend=hip_backend)
        assert sub.labels == ["x1", "x2"] and sub.grid.tobytes() == wsub.grid.tobytes() and sub.owner is None
        # the picture itself: all the mass of every variable, and every variable under its own mean
        bel = [(v.varType.manifold, iif.ppe_coords(v.varType.manifold, v.val), v.bw, (0, 1)) for v in map(fg.getVariable, got.labels)]
        ref = sc.scene_grid_numpy(bel, (96, 40), owner=True)
        scs.check_values(bel, got.grid, ref[0], None, "session")
        print(f"steps {got.extent[1]:.4f} {got.extent[3]:.4f}, tile_beliefs {got.tile_beliefs} of {scs.n_tiles((96, 40)) * n_vars}")
        assert got.at(*bel[0][1][:, :2].mean(axis=0)) in got.labels and got.at(1e6, 0.0) is None
