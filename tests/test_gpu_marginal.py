"""-m gpu: marginal densities on the device (nbp_run_marginal_grid / nbp_kde_marginal_grid / nbp_run_evaluate_marginal,
csrc/nbp_marginal.h) through the C ABI and through the mirror, held to the criteria of tests/marginal_cases.py: grids within 1e-12
relative (+ the clamp's floor) of the exact sums of marginal_grid_numpy, extents bit-equal to the numpy arithmetic, bit-equalities
where the definition promises them (a grid alone and in a batch, swapped coordinates, the full mask against nbp_run_evaluate).

Clouds come from ppe_cases.cloud; bandwidths are fitted with nbp_run_bandwidth where a belief holds more than two points and is
not all-identical, and set by hand otherwise."""
import ctypes as C

import numpy as np
import pytest

import marginal_cases as mc
import ppe_cases as pc
import query_cases as qc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
mg = iif.marginal
bq = iif.beliefquery


def _descriptors(items, beliefs, slots, seed):
    """every coordinate subset of every belief's manifold, the grid sizes cycling through marginal_cases.SIZES_*, explicit
    extents -> [(belief index, dims, n, extent)]"""
    rng = np.random.default_rng(seed)
    out, k1, k2 = [], 0, 0
    per_man = {}
    for i, (m, _, _) in enumerate(items):
        per_man.setdefault(m, []).append(i)
    turn = {m: 0 for m in per_man}
    for m in per_man:
        for dims in mc.subsets(m):
            i = per_man[m][turn[m] % len(per_man[m])]  # the clouds of the manifold take turns
            turn[m] += 1
            if len(dims) == 1:
                n, k1 = mc.SIZES_1D[k1 % len(mc.SIZES_1D)], k1 + 1
            else:
                n, k2 = mc.SIZES_2D[k2 % len(mc.SIZES_2D)], k2 + 1
            X, bw = beliefs[i]
            out.append((i, dims, n, mc.explicit_extent(m, X, bw, dims, n, rng)))
    return out


def _run_and_check(be, items, slots, mans, beliefs, descs, what):
    grids, ext = be.run_marginal_grid([(slots[i], mans[i], dims, n, e) for i, dims, n, e in descs], return_extent=True)
    for k, (i, dims, n, e) in enumerate(descs):
        X, bw = beliefs[i]
        assert np.array_equal(ext[k][:2 * len(dims)], e) and np.all(ext[k][2 * len(dims):] == 0)
        mc.check_grid(mans[i], X, bw, dims, n, np.asarray(e), grids[k], f"{what} [{k}] {items[i]}")
    return grids


@pytest.mark.parametrize("N", [64, 65, 200, 512])
def test_grid_every_manifold_every_subset(hip_backend, N):
    """all descriptors in ONE call; exact tiles, partial edge tiles and more than one tile per axis all occur"""
    items = [(m, kind, N) for m in qc.MANIFOLDS for kind in mc.KINDS]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = mc.load(be, items, 700 + N)
        descs = _descriptors(items, beliefs, slots, 710 + N)
        assert {n for _, d, n, _ in descs if len(d) == 1} == set(mc.SIZES_1D) and {n for _, d, n, _ in descs if len(d) == 2} == set(mc.SIZES_2D)
        assert {(mans[i], d) for i, d, _, _ in descs} == {(m, d) for m in qc.MANIFOLDS for d in mc.subsets(m)}
        _run_and_check(be, items, slots, mans, beliefs, descs, f"N={N}")
    finally:
        be.close()


def test_grid_counts_below_the_context_size(hip_backend):
    items = [(m, kind, c) for m in qc.MANIFOLDS for c in (1, 2, 63, 150) for kind in ("gaussian", "across_pi")]
    be = hip_backend(200, len(items))
    try:
        slots, mans, beliefs = mc.load(be, items, 721)
        rng = np.random.default_rng(722)
        descs = []
        for i, (m, kind, c) in enumerate(items):
            subs = mc.subsets(m)
            dims = subs[i % len(subs)]
            n = (17,) if len(dims) == 1 else (17, 33)
            descs.append((i, dims, n, mc.explicit_extent(m, *beliefs[i], dims, n, rng)))
        _run_and_check(be, items, slots, mans, beliefs, descs, "counts")
    finally:
        be.close()


def test_automatic_extent_and_mass(hip_backend):
    N, n = 200, 64
    cases = [(abi.EUCLID2, (0, 1))] * 3 + [(abi.EUCLID3, (0, 2))] * 2 + [(abi.EUCLID3, (2, 1))] + [(abi.SE2, (0, 1))] * 2 + [(abi.SE2, (1, 2)), (abi.SE2, (2, 0))]
    items = [(m, "gaussian", N) for m, _ in cases] + [(abi.SE2, "across_pi", N), (abi.CIRCULAR, "across_pi", N), (abi.EUCLID2, "across_pi", 150)]
    extra = [(abi.SE2, (2, 1)), (abi.CIRCULAR, (0,)), (abi.EUCLID2, (1, 0))]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = mc.load(be, items, 731)
        req = [(slots[i], m, dims, (n,) * len(dims), None, 4.0) for i, (m, dims) in enumerate(cases + extra)]
        grids, ext = be.run_marginal_grid(req, return_extent=True)
        left_out = 0
        for i, (m, dims) in enumerate(cases + extra):
            X, bw = beliefs[i]
            nn = (n,) * len(dims)
            want = mg.grid_extent_numpy(m, X, bw, dims, nn, 4.0)
            assert ext[i].tobytes() == want.tobytes(), (i, m, dims, ext[i], want)
            mc.check_grid(m, X, bw, dims, nn, want, grids[i], f"auto [{i}] {items[i]}")
            if i >= len(cases):
                continue
            mass = grids[i].sum() * ext[i][1] * ext[i][3]
            ok = all(ext[i][2 * a + 1] <= 0.7 * bw[d] for a, d in enumerate(dims))
            print(f"auto [{i}] manifold {m} dims {dims}: steps {ext[i][1]:.4f}, {ext[i][3]:.4f}, bw {bw}, precondition {ok}, mass {mass:.9f}")
            if not ok:
                left_out += 1
                continue
            assert mc.MASS_LO <= mass <= mc.MASS_HI, (i, mass)
        assert left_out * 10 <= len(cases), f"{left_out} of {len(cases)} clouds miss step <= 0.7 h"
        # 1-D with the automatic extent, n = 2 (the smallest a Euclidean axis takes) and a circular axis at n = 1
        g, e = be.run_marginal_grid([(slots[0], mans[0], (1,), (2,), None, 0.5), (slots[11], abi.CIRCULAR, (0,), (1,), None, 4.0)], return_extent=True)
        for k, (i, dims, nn, mar) in enumerate(((0, (1,), (2,), 0.5), (11, (0,), (1,), 4.0))):
            want = mg.grid_extent_numpy(mans[i], *beliefs[i], dims, nn, mar)
            assert e[k].tobytes() == want.tobytes()
            mc.check_grid(mans[i], *beliefs[i], dims, nn, want, g[k], f"auto small [{k}]")
    finally:
        be.close()


def test_a_grid_alone_is_its_value_in_a_batch_of_40(hip_backend):
    N = 200
    rng = np.random.default_rng(741)
    items = [(qc.MANIFOLDS[rng.integers(5)], mc.KINDS[rng.integers(4)], int(rng.choice([N, N, 150, 63, 2, 1]))) for _ in range(40)]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = mc.load(be, items, 742)
        descs = []
        for i, (m, kind, c) in enumerate(items):
            subs = mc.subsets(m)
            dims = subs[rng.integers(len(subs))]
            n = mc.SIZES_1D[rng.integers(3)] if len(dims) == 1 else mc.SIZES_2D[rng.integers(5)]
            descs.append((i, dims, n, mc.explicit_extent(m, *beliefs[i], dims, n, rng)))
        req = [(slots[i], mans[i], dims, n, e) for i, dims, n, e in descs]
        batch = be.run_marginal_grid(req)
        again = be.run_marginal_grid(req)
        for k in range(len(req)):
            assert batch[k].tobytes() == again[k].tobytes()
            if k % 4 == 0:
                assert be.run_marginal_grid([req[k]])[0].tobytes() == batch[k].tobytes(), (k, descs[k])
        # the same slot in two descriptors of one call, the second with the automatic extent equal to the first's explicit one
        two = [k for k, (i, dims, n, e) in enumerate(descs) if len(dims) == 2 and min(n) >= 2 and items[i][2] >= 63][:3]
        assert two
        for k in two:
            i, dims, n, e = descs[k]
            a, b = be.run_marginal_grid([req[k], req[k]])
            assert a.tobytes() == b.tobytes() == batch[k].tobytes()
            # swapped coordinates: the transpose, bit for bit
            t = be.run_marginal_grid([(slots[i], mans[i], dims[::-1], n[::-1], [e[2], e[3], e[0], e[1]])])[0]
            assert np.ascontiguousarray(t.T).tobytes() == batch[k].tobytes(), (k, descs[k])
        # dims = (1, 0) against (0, 1) on a fresh Euclid(2) grid that spans several tiles
        j = next(i for i, it in enumerate(items) if abi.MANIFOLD_DIM[it[0]] >= 2 and it[2] >= 63)
        e = mc.explicit_extent(mans[j], *beliefs[j], (0, 1), (64, 33), rng)
        g01, g10 = be.run_marginal_grid([(slots[j], mans[j], (0, 1), (64, 33), e), (slots[j], mans[j], (1, 0), (33, 64), [e[2], e[3], e[0], e[1]])])
        assert g01.tobytes() == np.ascontiguousarray(g10.T).tobytes()
        # explicit extent equal to the automatic one: the same bits
        ga, ea = be.run_marginal_grid([(slots[j], mans[j], (0, 1), (33, 17), None, 3.0)], return_extent=True)
        ge = be.run_marginal_grid([(slots[j], mans[j], (0, 1), (33, 17), ea[0])])[0]
        assert ga[0].tobytes() == ge.tobytes()
    finally:
        be.close()


def test_evaluate_marginal(hip_backend):
    N = 200
    items = [(m, kind, c) for m in qc.MANIFOLDS for kind, c in (("gaussian", N), ("across_pi", 63))]
    be = hip_backend(N, len(items))
    try:
        slots, mans, beliefs = mc.load(be, items, 751)
        rng = np.random.default_rng(752)
        Q = [qc.make_queries(m, X, bw, qc.TILE + 1, rng) for m, (X, bw) in zip(mans, beliefs)]
        full = [(1 << abi.MANIFOLD_DIM[m]) - 1 for m in mans]
        want = be.run_evaluate(slots, mans, Q)
        got = be.run_evaluate_marginal(slots, mans, full, Q)
        for i in range(len(items)):
            assert got[i].tobytes() == want[i].tobytes(), (i, items[i])
        # proper subsets, all in one call, at queries without the 40 h ones (whose every term is the clamp's, not the density's)
        Qn = [q[np.arange(len(q)) % 4 != 2] for q in Q]
        req = [(i, K) for i, m in enumerate(mans) for K in range(1, full[i]) if abi.MANIFOLD_DIM[m] > 1]
        dev = be.run_evaluate_marginal([slots[i] for i, _ in req], [mans[i] for i, _ in req], [K for _, K in req], [Qn[i] for i, _ in req])
        for (i, K), d in zip(req, dev):
            dims = [b for b in range(3) if K >> b & 1]
            ref = mg.marginal_density_numpy(mans[i], *beliefs[i], dims, Qn[i])
            rel = np.max(np.abs(d - ref) / ref)
            print(f"[{i}] {items[i]} mask {K}: max |dev - ref| / ref = {rel:.3e}")
            assert np.all(np.abs(d - ref) <= mc.DENS_RTOL * ref), (i, K, rel)
            assert be.run_evaluate_marginal([slots[i]], [mans[i]], [K], [Qn[i][5:6]])[0][0] == d[5]
        # against the grid kernel at the grid's own points: 2 DENS_RTOL, relative.  Where a grid point lies so far from every
        # particle that the value itself is of the order of the clamp of exp_nonpos (a wrapped across_pi cloud on a Euclidean
        # axis: the middle of the grid is > 37 h from both ends), the two forms meet the clamp differently -- one clamped
        # exponential per particle there, a product of two per-axis ones here: the floor of marginal_cases, and nothing else
        greq, gq = [], []
        for i, m in enumerate(mans):
            for dims in mc.subsets(m)[::2]:
                n = (33,) if len(dims) == 1 else (17, 33)
                e = mc.explicit_extent(m, *beliefs[i], dims, n, rng)
                greq.append((slots[i], m, dims, n, e))
                gq.append(mc.grid_points(m, mg.grid_axes(np.asarray(e), n), dims))
        grids = be.run_marginal_grid(greq)
        pts = be.run_evaluate_marginal([g[0] for g in greq], [g[1] for g in greq], [sum(1 << d for d in g[2]) for g in greq], gq)
        for g, a, b in zip(greq, grids, pts):
            a = a.reshape(-1)
            rel = np.max(np.abs(a - b) / np.maximum(b, 1e-280))
            print(f"grid against points, manifold {g[1]} dims {g[2]}: max relative difference {rel:.3e}")
            fl = mc.floor(len(beliefs[slots.index(g[0])][0]), beliefs[slots.index(g[0])][1], g[2])
            assert np.all(np.abs(a - b) <= 2 * mc.DENS_RTOL * b + fl), (g[:4], rel)
            big = b > 1e-280
            assert big.any() and np.all(np.abs(a - b)[big] <= 2 * mc.DENS_RTOL * b[big]), (g[:4], rel)
    finally:
        be.close()


def test_partial_belief(hip_backend):
    N = 100
    be = hip_backend(N, 3)
    rng = np.random.default_rng(761)
    try:
        X = pc.cloud("gaussian", abi.SE2, N, rng)
        bw = np.array([0.3, 0.4, 0.0])
        be.beliefs_write([1], [abi.SE2], [(pc.to_points(abi.SE2, X), bw, None)])
        pts, bwb, _ = be.beliefs_read([1], [abi.SE2])[0]
        X = coords(abi.SE2, pts)
        assert np.array_equal(bwb, bw)
        assert np.isnan(be.run_evaluate([1], [abi.SE2], [X[:5]])[0]).all()  # unchanged: all coordinates enter there
        for dims, n in (((0, 1), (17, 33)), ((1, 0), (16, 16)), ((0,), (17,)), ((1,), (257,))):
            e = mc.explicit_extent(abi.SE2, X, bw, dims, n, rng)
            g = be.run_marginal_grid([(1, abi.SE2, dims, n, e)])[0]
            mc.check_grid(abi.SE2, X, bw, dims, n, np.asarray(e), g, "partial")
            ga, ea = be.run_marginal_grid([(1, abi.SE2, dims, n, None, 4.0)], return_extent=True)
            assert ea[0].tobytes() == mg.grid_extent_numpy(abi.SE2, X, bw, dims, n).tobytes() and np.isfinite(ga[0]).all()
        d = be.run_evaluate_marginal([1], [abi.SE2], [3], [X[:7]])[0]
        ref7 = mg.marginal_density_numpy(abi.SE2, X, bw, (0, 1), X[:7])
        assert np.all(np.abs(d - ref7) <= mc.DENS_RTOL * ref7)
        for dims, n in (((2,), (17,)), ((0, 2), (17, 33)), ((2, 1), (33, 2))):
            g = be.run_marginal_grid([(1, abi.SE2, dims, n, [0.0, 0.1] * len(dims))])[0]
            assert g.shape == n and np.isnan(g).all(), dims
            assert np.isnan(be.run_marginal_grid([(1, abi.SE2, dims, n, None, 4.0)])[0]).all()
        for K in (4, 5, 6, 7):
            assert np.isnan(be.run_evaluate_marginal([1], [abi.SE2], [K], [X[:5]])[0]).all()
        # the mirror: a partial belief defaults to its partial coordinates, through slot 0
        b = iif.Belief(abi.SE2, pts, bw)
        g, axes = b.marginal((1, 2)).grid((17, 33), backend=be)
        ref, ext = mg.marginal_grid_numpy(abi.SE2, X, bw, (0, 1), (17, 33))
        assert np.array_equal(axes[0], mg.grid_axes(ext, (17, 33))[0]) and np.array_equal(axes[1], mg.grid_axes(ext, (17, 33))[1])
        assert np.all(np.abs(g - ref) <= mc.DENS_RTOL * ref + mc.floor(N, bw, (0, 1)))
        p = b.marginal((1, 2))(pts[:7], backend=be)
        assert np.all(np.abs(p - ref7) <= mc.DENS_RTOL * ref7)
    finally:
        be.close()


def test_refusals_name_the_descriptor(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rng = np.random.default_rng(771)
    try:
        X = pc.cloud("gaussian", abi.SE2, 64, rng)
        be.beliefs_write([0, 1], [abi.SE2, abi.EUCLID2], [(pc.to_points(abi.SE2, X), [0.3, 0.3, 0.2], None), (X[:, :2], [0.3, 0.3], None)])
        good = (0, abi.SE2, (0, 1), (5, 6), [0.0, 0.1, 0.0, 0.1])
        bad = [
            (4, abi.SE2, (0, 1), (5, 6), [0, 0.1, 0, 0.1]),            # a slot outside the context
            (1, abi.EUCLID2, (2,), (5,), [0, 0.1]),                    # a coordinate outside the manifold
            (1, abi.EUCLID2, (0, 2), (5, 6), [0, 0.1, 0, 0.1]),
            (0, abi.SE2, (-1,), (5,), [0, 0.1]),
            (0, abi.SE2, (1, 1), (5, 6), [0, 0.1, 0, 0.1]),            # a repeated coordinate
            (0, abi.SE2, (0, 1), (0, 6), [0, 0.1, 0, 0.1]),            # n outside 1 .. NBP_GRID_MAX
            (0, abi.SE2, (0, 1), (5, abi.GRID_MAX + 1), [0, 0.1, 0, 0.1]),
            (0, abi.SE2, (0,), (1,), None, 4.0),                       # n < 2 on a Euclidean axis with the automatic extent
            (0, abi.SE2, (2, 1), (1, 1), None, 4.0),
            (0, abi.SE2, (0, 1), (5, 6), [np.nan, 0.1, 0, 0.1]),       # a non-finite lo / step / margin
            (0, abi.SE2, (0, 1), (5, 6), [0, 0.1, 0, np.inf]),
            (0, abi.SE2, (0, 1), (5, 6), None, np.nan),
            (0, abi.SE2, (0,), (5,), None, -np.inf),
        ]
        for b in bad:
            for pos in (0, 2):
                req = [good] * pos + [b] + [good]
                with pytest.raises(iif.NbpError, match=rf"-4.*descriptor {pos}\b"):
                    be.run_marginal_grid(req)
        # offsets that do not match the grid sizes
        g = (abi.GridDesc * 2)(be._grid_desc(*good), be._grid_desc(*good))
        out, ext = (C.c_double * 64)(), (C.c_double * 8)()
        assert lib.nbp_run_marginal_grid(ctx, g, 2, (C.c_int32 * 3)(0, 30, 60), out, ext) == 0
        for first, pos in (((0, 30, 59), 1), ((0, 31, 61), 0), ((1, 31, 61), 0), ((0, 30, 29), 1)):
            assert lib.nbp_run_marginal_grid(ctx, g, 2, (C.c_int32 * 3)(*first), out, ext) == -4
            assert f"descriptor {pos}".encode() in lib.nbp_last_error()
        assert lib.nbp_run_marginal_grid(ctx, g, 2, (C.c_int32 * 3)(0, 30, 60), out, None) == 0   # extent_out may be NULL
        assert lib.nbp_run_marginal_grid(ctx, None, 0, None, None, None) == 0                    # n = 0 is NBP_OK
        assert lib.nbp_run_marginal_grid(None, g, 2, (C.c_int32 * 3)(0, 30, 60), out, ext) == -1
        assert lib.nbp_run_marginal_grid(ctx, g, 2, None, out, ext) == -1
        assert lib.nbp_run_marginal_grid(ctx, g, 2, (C.c_int32 * 3)(0, 30, 60), None, ext) == -1
        with pytest.raises(iif.NbpError, match="-1"):
            be.run_marginal_grid([(0, 9, (0,), (5,), [0, 0.1])])  # an unknown manifold is an argument error, as everywhere
        # the masks of run_evaluate_marginal
        for K, m in ((0, abi.SE2), (8, abi.SE2), (4, abi.EUCLID2), (2, abi.CIRCULAR), (-1, abi.SE2)):
            for pos in (0, 1):
                with pytest.raises(iif.NbpError, match=rf"-4.*belief {pos}\b"):
                    be.run_evaluate_marginal([0] * pos + [1 if m == abi.EUCLID2 else 0], [abi.SE2] * pos + [m], [7] * pos + [K], [X[:2]] * (pos + 1))
        with pytest.raises(iif.NbpError, match="-4"):
            be.run_evaluate_marginal([4], [abi.SE2], [1], [X[:2]])
        with pytest.raises(iif.NbpError, match="-4"):
            be.kde_marginal_grid(abi.EUCLID2, X[:, :2], [0.3, 0.3], (0, 2), (5, 6), [0, 0.1, 0, 0.1])
        # the context stays usable, and nothing was launched on the refused calls' behalf: slot 0 still holds its belief
        grid = be.run_marginal_grid([good])[0]
        mc.check_grid(abi.SE2, coords(abi.SE2, be.beliefs_read([0], [abi.SE2])[0][0]), np.array([0.3, 0.3, 0.2]), (0, 1), (5, 6),
                      np.array(good[4]), grid, "after refusals")
        assert np.isfinite(be.run_evaluate_marginal([0], [abi.SE2], [5], [X[:3]])[0]).all()
    finally:
        be.close()


def test_session_serves_all_variables_without_moving_a_belief(hip_backend):
    fg = qc.chain6(5)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=71)
        before = {k: ses.stats[k] for k in ("uploads", "readbacks")}
        got = ses.marginalGrid(dims=(1,), n=64)
        assert {k: ses.stats[k] for k in before} == before
        assert list(got) == fg.ls() and len(got) == 6
        for v in fg.ls():
            var = fg.getVariable(v)
            grid, axes = got[v]
            ref, ext = mg.marginal_grid_numpy(abi.EUCLID1, fg.getVal(v), var.bw, (0,), (64,), margin=4.0)
            assert np.array_equal(axes[0], mg.grid_axes(ext, (64,))[0])
            assert np.all(np.abs(grid - ref) <= mc.DENS_RTOL * ref + mc.floor(len(var.val), var.bw, (0,))), v
            assert abs(grid.sum() * ext[1] - 1) <= 2e-4
        one = ses.marginalGrid(["x3"], dims=(1,), n=64)
        assert list(one) == ["x3"] and one["x3"][0].tobytes() == got["x3"][0].tobytes()
        assert {k: ses.stats[k] for k in before} == before
        # the host-buffer form (nbp_kde_marginal_grid, a context of its own): the same bits
        g, axes = iif.marginalGrid(fg, "x3", (1,), 64, backend=hip_backend)
        assert g.tobytes() == got["x3"][0].tobytes() and np.array_equal(axes[0], got["x3"][1][0])
        g, _ = iif.marginalGrid(fg, "x3", None, 64, margin=4.0, backend=iif.HipBackend)
        assert g.tobytes() == got["x3"][0].tobytes()
