"""-m gpu: heatmap densities on the HIP library (tests/heatmap_cases.py) -- stage by stage through the C ABI against the numpy
restatement, through the mirror (HeatmapGridDensity / LevelSetGridNormal / PartialPriorPassThrough.fromDensity), the known
answers, the refusals.  The largest grid is 300 x 257."""
import ctypes as C

import numpy as np
import pytest

import heatmap_cases as hc
import sampling_cases as sc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
hm = iif.heatmap


@pytest.fixture(scope="module")
def be(hip_backend):
    b = hip_backend(hc.N_CTX, 4)
    yield b
    b.close()


def run(be, case, M=None, n=None, seed=None, seed2=None, jitter=0, slot=-1):
    """create, build, draw, destroy -> (total, cell, pre, d, W, wtotal, pick, points, bw)"""
    h = be.heatmap_create(case["data"], case["x"], case["y"], case.get("bw_factor", 0.7))
    try:
        assert be.heatmap_info(h)[3] == 0
        cell, pre, d, W = be.heatmap_build(h, case["M"] if M is None else M, case["seed"] if seed is None else seed)
        bw, total, wtotal, Mi = be.heatmap_info(h)
        assert Mi == len(cell)
        pick, pts, bw2 = be.heatmap_draw(h, case["n"] if n is None else n, case["seed2"] if seed2 is None else seed2, jitter=jitter, slot=slot)
        assert np.array_equal(bw, bw2)
        return total, cell, pre, d, W, wtotal, pick, pts, bw
    finally:
        be.heatmap_destroy(h)


@pytest.mark.parametrize("case", hc.STAGE_CASES, ids=[c["name"] for c in hc.STAGE_CASES])
def test_stages_against_the_restatement(be, case):
    hc.check_stages(case, hc.restate(case), *run(be, case))


def test_every_M_and_n_on_one_grid(be):
    """M in {1, 63, 64, 65, 120, 1000, 10000} x n in {1, 120, N} on the 20 x 20 grid: the sums and the searches over the weights at
    every size.  (Index equality with the restatement is asked for in the decidable cases above; here the device's own stages must
    agree with one another, whatever the margins.)"""
    case = hc.STAGE_CASES[2]
    h = be.heatmap_create(case["data"], case["x"], case["y"])
    try:
        for M in (1, 63, 64, 65, 120, 1000, 10000):
            cell, pre, d, W = be.heatmap_build(h, M, seed=M)
            R = hc.restate(case, M=M, n=1, seed=M)
            assert np.array_equal(cell, R["cell"]), M  # (cdf and the draws are bit-equal on both sides: equal whatever the margin)
            assert np.all(np.abs(pre - R["pre"]) <= hc.pre_tol(case, R)), M
            _, total, wtotal, Mi = be.heatmap_info(h)
            assert Mi == M and total == R["total"] and wtotal == hm.scan_numpy(W)[-1], M
            wcdf = hm.scan_numpy(W)
            for n in (1, 120, hc.N_CTX):
                pick, pts, _ = be.heatmap_draw(h, n, seed=7 * M + n)
                ua, _ = hm.uniform_pairs(7 * M + n, np.arange(n), hm.PURP_HMPICK, 0)
                assert np.array_equal(pick, hm.search_numpy(wcdf, ua * wtotal)), (M, n)  # (the device's own W: the same sums)
                assert np.array_equal(pts, pre[pick]), (M, n)
    finally:
        be.heatmap_destroy(h)


def test_mirror_is_the_abi(be, hip_backend):
    case = hc.STAGE_CASES[3]
    total, cell, pre, d, W, wtotal, pick, pts, bw = run(be, case, seed2=case["seed"])
    Z = iif.HeatmapGridDensity(case["data"], (case["x"], case["y"]), None, 0.7, N=case["M"], n=case["n"], seed=case["seed"], backend=hip_backend)
    assert np.array_equal(Z.points, pts) and np.array_equal(Z.bw, bw) and Z.bw_factor == 0.7 and Z.data.shape == (20, 20)
    L = iif.LevelSetGridNormal(case["data"], (case["x"], case["y"]), 5.5, 0.1, N=case["M"], n=case["n"], seed=case["seed"], backend=be)
    assert np.array_equal(L.heatmap.points, pts) and (L.level, L.sigma, L.sigma_scale) == (5.5, 0.1, 3.0)
    # hgd(pts): the KDE of (points, bw)
    Q = np.stack([np.linspace(100.0, 138.0, 7), np.linspace(-7.0, 31.0, 7)], axis=1)
    ref = iif.density_numpy(abi.EUCLID2, Z.points, Z.bw, Q)
    got = Z(Q)
    assert np.all(np.abs(got - ref) <= hc.W_RTOL * ref + 1e-300), (got, ref)
    # sample(hgd, n, seed): the jittered draw of the ABI
    _, _, _, _, _, _, jp, jpts, _ = run(be, case, n=50, seed2=99, jitter=1)
    assert np.array_equal(iif.sample(Z, 50, 99), jpts) and np.array_equal(hm.sample(L, 50, 99), jpts)
    assert np.abs((jpts - pre[jp]) / bw).max() < 6 and not np.array_equal(jpts, pre[jp])


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seeds", hc.GAUSS_SEEDS)
def test_gaussian_image_within_the_reference_bands(be, seeds):
    img, x, y = hc.gaussian_image()
    Z = iif.HeatmapGridDensity(img, (x, y), None, 0.07, N=1000, seed=seeds[0], backend=be)
    hc.gaussian_bands_ok(Z.sample(1000, seeds[1]), f"device, seeds {seeds}")


def test_cell_picks_follow_the_field(be):
    case, p = hc.cells_field()
    cell = run(be, case, M=hc.CELLS_M, n=1, seed=hc.CELLS_SEED)[1]
    sc.chi2_ok(np.bincount(cell, minlength=p.size), p, "cell picks on the 20 x 20 grid (device)")


def test_picks_concentrate_like_exp_minus_d(be):
    d, x, y = hc.bowl()
    case = dict(data=d, x=x, y=y)
    _, _, pre, _, W, wtotal, pick, pts, bw = run(be, case, M=hc.BOWL_M, n=hc.BOWL_N, seed=hc.BOWL_SEED, seed2=hc.BOWL_SEED + 1)
    sc.chi2_ok(np.bincount(pick, minlength=hc.BOWL_M), W / W.sum(), "picks on the bowl (device)")
    assert W.min() < 0.05 and np.array_equal(pts, pre[pick])
    _, _, pre, _, _, _, pick, pts, bw = run(be, case, M=hc.BOWL_M, n=hc.BOWL_N, seed=hc.BOWL_SEED, seed2=hc.BOWL_SEED + 1, jitter=1)
    sc.gaussian_ok((pts - pre[pick]) / bw, [0.0, 0.0], np.eye(2), "jitter on the device")


# ---- the pass-through path -----------------------------------------------------------------------------------------------------------
def test_passthrough_prior_from_a_heatmap(be, hip_backend):
    """testSpecialEuclidean2Mani.jl:331-369 with a real heatmap: the belief IS the density"""
    img, x, y = hc.levelset_image()
    Z = iif.LevelSetGridNormal(img, (x, y), 5.5, 0.1, N=120, backend=be)
    assert Z.heatmap.points.shape == (120, 2)
    h = 0.7 * 0.5 * (2.0 + 2.0)
    np.testing.assert_array_equal(Z.heatmap.bw, [h, h])
    fg = hc.graph_w_priors(Z)
    (pts, bw), ipc = iif.propagateBelief(fg, "x0", ["x0f1"], backend=hip_backend, seed=5)
    assert pts.shape == (120, 6)
    np.testing.assert_array_equal(pts[:, :2], Z.heatmap.points)
    np.testing.assert_array_equal(np.arctan2(pts[:, 3], pts[:, 2]), np.zeros(120))
    np.testing.assert_array_equal(bw, [h, h, 0.0])


def test_draw_into_a_slot_is_the_draw_to_the_host(be):
    case = hc.STAGE_CASES[3]
    for n in (1, 120, hc.N_CTX):
        for jitter in (0, 1):
            be.belief_write(2, abi.EUCLID2, np.full((hc.N_CTX, 2), 9.0), np.ones(2), np.ones(2))  # (what the draw must replace)
            pts, bw = run(be, case, n=n, jitter=jitter, slot=2)[7:9]
            got, gbw, gipc = be.belief_read(2, abi.EUCLID2)
            assert got.shape == (n, 2) and np.array_equal(got, pts), (n, jitter)
            assert np.array_equal(gbw, bw) and np.array_equal(gipc, [0.0, 0.0])
            raw, _ = be.slot_read(2, abi.EUCLID2)
            assert np.all(raw[n:] == 0.0)
    h = be.heatmap_create(case["data"], case["x"], case["y"])
    try:
        be.heatmap_build(h, 100, 1, outputs=False)
        assert be.heatmap_draw(h, 10, 3, slot=1, outputs=False)[2][0] == be.heatmap_info(h)[0][0]
        assert np.array_equal(be.belief_read(1, abi.EUCLID2)[0], be.heatmap_draw(h, 10, 3)[1])
    finally:
        be.heatmap_destroy(h)


def test_solve_with_a_heatmap_prior(be, hip_backend):
    """the "w Relative" graph (:456-527): the solve runs and x1 stays at its prior"""
    img, x, y = hc.levelset_image()
    fg = hc.graph_w_relative(iif.LevelSetGridNormal(img, (x, y), 5.5, 0.1, N=120, backend=be))
    iif.initAll(fg, backend=hip_backend, seed=11)
    iif.solveTree(fg, backend=hip_backend, seed=12)
    for v in ("x0", "x1"):
        val = fg.getVariable(v).val
        assert val.shape == (hc.N_CTX, 6) and np.all(np.isfinite(val))
    v1 = fg.getVariable("x1").val
    c1 = np.stack([v1[:, 0], v1[:, 1], np.arctan2(v1[:, 3], v1[:, 2])], axis=1)
    assert np.abs(c1.mean(axis=0)).max() < 0.1


# ---- refusals and the life of a handle -------------------------------------------------------------------------------------------------
def test_refusals(be):
    x = np.linspace(0.0, 1.0, 5)
    ok = np.ones((5, 5))
    bad = [(ok, x ** 2 + x, x), (ok, x, x[::-1].copy()), (ok, x, np.array([0.0, 0.25, 0.5, 0.75, 1.0 + 1e-8])),
           (np.ones((1, 5)), x[:1], x), (np.ones((5, 1)), x, x[:1]), (np.where(np.eye(5) > 0, np.nan, 1.0), x, x),
           (np.where(np.eye(5) > 0, -np.inf, 1.0), x, x), (-ok, x, x), (np.zeros((5, 5)), x, x)]
    for data, xx, yy in bad:
        with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:"):
            be.heatmap_create(data, xx, yy)
    with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:"):
        be.heatmap_create(ok, x, x, bw_factor=0.0)
    # nx * ny > 2^26: the sizes alone, looked at before the pointers
    out = C.c_void_p()
    assert be.lib.nbp_heatmap_create(be._ctx, None, 8193, 8192, None, None, 0.7, C.byref(out)) == abi.ERR_INVALID and not out
    assert b"2^26" in be.lib.nbp_last_error()
    h = be.heatmap_create(ok, x, x)
    try:
        with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:.*build"):
            be.heatmap_draw(h, 10, 1)  # a draw before a build
        for M in (0, -3):
            with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:"):
                be.heatmap_build(h, M, 1)
        be.heatmap_build(h, 50, 1, outputs=False)
        with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:.*at most N"):
            be.heatmap_draw(h, be.N + 1, 1, slot=0)
        assert be.heatmap_draw(h, be.N + 1, 1)[1].shape == (be.N + 1, 2)  # without a slot n is free
        with pytest.raises(iif.NbpError):
            be.heatmap_draw(h, 10, 1, slot=be.n_slots)
        with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:"):
            be.heatmap_draw(h, 0, 1)
    finally:
        be.heatmap_destroy(h)


def test_rebuild_replaces_and_a_handle_outlives_its_context(hip_backend):
    case = hc.STAGE_CASES[2]
    b = hip_backend(64, 2)
    h = b.heatmap_create(case["data"], case["x"], case["y"])
    first = b.heatmap_build(h, 300, 1)
    second = b.heatmap_build(h, 40, 2)
    again = b.heatmap_build(h, 300, 1)
    assert len(second[0]) == 40 and b.heatmap_info(h)[3] == 300
    for a, c in zip(first, again):
        assert np.array_equal(a, c)
    b.close()  # the context goes first: the heatmap's device memory goes with it, the handle stays valid for destroy
    with pytest.raises(iif.NbpError):
        b.heatmap_build(h, 10, 1)
    b.heatmap_destroy(h)
