"""Shared cases of the heatmap-density tests (tests/test_heatmap.py on the CPU: the numpy restatement alone; tests/test_gpu_heatmap.py
on the device: the C ABI and the mirror): the grids, the sizes, the seeds and the criteria, written once.

The criteria, stage by stage, for a device run against `heatmap_density_numpy` (R) on the same inputs and seeds:

  total      bit-equal to R's (cdf itself stays on the device: total = cdf[-1] is what the ABI shows of it; the crafted cell counts
             put a segment, a tile and a group of tiles one element past full, so every level of the sum ends in `total`).
  cell       equal.
  pre        |dev - R| <= BM_ATOL * h + EPS * |h n| + EPS * |p| per coordinate.  BM_ATOL = 1e-14 is what tests/test_nbp_math.py
             (test_box_muller_pair) holds the shared Box-Muller to against libm, absolute on a standard normal; times h it is the
             difference the two normals can make.  p = x + h * n is then rounded twice on either side (the product, the sum), half
             an ulp each: EPS * |h n| and EPS * |p| with EPS = 2^-52.  (Without these two terms the bound would ask for bits the
             two libms do not share: h * 1e-14 is below an ulp of p wherever |p| > 45 h.)
  d          that, through the bilinear formula: |dev - R| <= Gx (tol_x / dx + 2 EPS nx) + Gy (tol_y / dy + 2 EPS ny) + 8 EPS max|data|,
             Gx / Gy = the largest difference of the field between neighbours along x / y (the interpolant's slope is at most
             G / spacing; the cell coordinate (p - x0) / dx carries an ulp of up to nx; the formula's seven operations round on
             values below max|data|).  Points inside the box on one side and outside on the other cannot be compared: the margins.
  W          relative DENS_RTOL (tests/marginal_cases.py: 1e-12, what the project holds exp_nonpos to) against
             exp(max(-(d - min d), -700)) of the DEVICE's d -- the exponential and the minimum alone; and against R's W with what a
             difference of d and of dmin adds, W (d_tol + max d_tol).
  wtotal     bit-equal to scan_numpy of the device's W.
  pick       equal.
  points     pre[pick] of the device bit for bit (jitter = 0).

Index equality is decidable only away from a boundary: `margins` computes, from R, how far every draw lies from the ends of its
CDF interval (relative to the total) and every pre-sample from the lines of its grid cell and the sides of the box (relative to
the spacing).  A seed is used only if all of them exceed MARGIN = 1e-9; test_heatmap.py asserts that for every case below, so
the device test leaves nothing out."""
import numpy as np

import marginal_cases as mc
from parity_utils import iif

hm = iif.heatmap
BM_ATOL = 1e-14  # tests/test_nbp_math.py::test_box_muller_pair
EPS = 2.0 ** -52
W_RTOL = mc.DENS_RTOL
MARGIN = 1e-9
SEED3R = 2  # of the 65 x 4161 grid
N_CTX = 150  # the context's N of the device tests (the pass-through case of the reference runs its solver with N = 150 here)


def _field(nx, ny, seed, nonpositive=0.0, offset=0.0):
    rng = np.random.default_rng(seed)
    data = rng.uniform(0.1, 2.0, (nx, ny))
    if nonpositive:
        bad = rng.uniform(size=(nx, ny)) < nonpositive
        data[bad] = np.where(rng.uniform(size=bad.sum()) < 0.5, 0.0, -rng.uniform(0.1, 1.0, bad.sum()))
    return data + offset


def _case(name, nx, ny, xr, yr, M, n, seed, **kw):
    return dict(name=name, data=_field(nx, ny, 100 + nx * ny, **kw), x=np.linspace(xr[0], xr[1], nx), y=np.linspace(yr[0], yr[1], ny),
                M=M, n=n, seed=seed, seed2=seed + 1000)


# 17 x 241 = 4097 = 64 * 64 + 1: one more than a multiple of the segment (64) and of the tile (4096), the block sizes of the two
# levels a sum of this length has.  The third and the fourth level (more than 64 and more than 4096 tiles: 64^3 + 1 and 2^24 + 1
# cells) are LEVEL_CASES below; the sum and the search by themselves, at every boundary of every level up to 2^26 elements, are
# tests/test_gpu_heatmap_scan.py (nbp_heatmap_scan_eval / nbp_heatmap_search_eval against scan_numpy / search_numpy), and
# test_heatmap.py ties scan_numpy to a wave-by-wave walk of the kernels before the device is compared with it.
STAGE_CASES = [
    _case("2 x 2", 2, 2, (-1.0, 1.0), (0.0, 3.0), M=1, n=1, seed=1),
    _case("3 x 2", 3, 2, (0.0, 1.0), (-2.0, -1.0), M=63, n=1, seed=1),
    _case("20 x 20, a third of the cells <= 0", 20, 20, (-9.5, 9.5), (-9.5, 9.5), M=64, n=120, seed=1, nonpositive=1.0 / 3.0),
    _case("20 x 20, x in [100, 138]", 20, 20, (100.0, 138.0), (-7.0, 31.0), M=65, n=N_CTX, seed=1, nonpositive=1.0 / 3.0),
    _case("20 x 20, field + 800", 20, 20, (100.0, 138.0), (-50.0, -12.0), M=1000, n=120, seed=1, offset=800.0),
    _case("201 x 201", 201, 201, (-10.0, 10.0), (-10.0, 10.0), M=120, n=120, seed=1),
    _case("300 x 257", 300, 257, (-3.0, 26.9), (5.0, 30.6), M=1000, n=N_CTX, seed=2, nonpositive=0.1),
    _case("17 x 241 = 64^2 + 1 cells", 17, 241, (0.0, 1.6), (100.0, 124.0), M=10000, n=120, seed=1),
]


# ---- the third and the fourth level of the sum through the real path (built on first use: the large ones are 134 MB and more) -----
# Which lengths reach what.  nbp_hm_scan_tiles_kernel forms a P3 carry from 65 tiles on (n > 64^3) and a P4 carry from 4097 tiles
# on (n > 2^24), but a carry is the one INTO the next segment: the first element whose sum contains the P3 carry of the tile totals
# is element 64 of tile 65 (n >= 64^3 + 64^2 + 64 + 1), and the first that contains a P4 carry is element 64 of tile 4161
# (n >= 2^24 + 64^3 + 64^2 + 64 + 1).  At 64^3 + 1 and 2^24 + 1 cells the kernel computes the carry and nothing reads it.  So each
# level has two grids: the first length with the extra level, and one some tiles past the first element that depends on it.
LEVEL3_CELLS, LEVEL4_CELLS = 64 ** 3 + 1, 2 ** 24 + 1
LEVEL3_READ, LEVEL4_READ = 64 ** 3 + 64 ** 2 + 64, 2 ** 24 + 64 ** 3 + 64 ** 2 + 64  # the first element that reads the P3 / P4 carry
LEVEL4_M = 100_000
PRE_LEVEL3_MS, PRE_LEVEL3_N = (64 ** 3 + 1, 64 ** 3 + 2 * 64 ** 2 + 1), 200_000  # the pre-sample axis: STAGE_CASES[2], 65 and 67 tiles of weights

# Which margins the level-3 grids need: `cell` needs none -- the device's cdf is scan_numpy's bit for bit (asserted on its own in
# test_gpu_heatmap_scan.py) and ua * total is the same product on both sides, so the two searches see the same bits (the argument
# of test_every_M_and_n_on_one_grid).  Nor could a seed provide one: a cell is 3.8e-6 of the total wide, so each of the 10^5 draws
# lies within 1e-9 of an end of its interval with probability 5e-4, about 50 of them on any seed.  `pre` -> `d` needs the grid
# margin (a point an ulp across a grid line or a side of the box reads another cell) and `pick` needs its own (the device's W are
# the restatement's to W_RTOL only, so wcdf differs in its last bits): test_heatmap.py asserts those two.


def _level3_grid():
    """65 x 4033 = 64^3 + 1 cells (65 tiles), a tenth of them <= 0, M = 100 000: every stage as for STAGE_CASES"""
    return _case("65 x 4033 = 64^3 + 1 cells", 65, 4033, (-3.2, 3.2), (0.0, 403.2), M=100_000, n=N_CTX, seed=2, nonpositive=0.1)


def _level3_grid_read():
    """65 x 4161 = 270 465 cells (67 tiles): the cells from 266 304 on, 1.5 % of them, lie behind the P3 carry"""
    return _case("65 x 4161: 67 tiles", 65, 4161, (-3.2, 3.2), (0.0, 416.0), M=100_000, n=N_CTX, seed=SEED3R, nonpositive=0.1)


def _level4(nx, ny, name, zero_cols):
    data = np.random.default_rng(100 + nx * ny).uniform(0.1, 2.0, (nx, ny))
    data[100:120] = -data[100:120]
    if zero_cols:
        data[:, ny - zero_cols:] = 0.0
    return dict(name=name, data=data, x=np.linspace(-12.8, 12.8, nx), y=np.linspace(0.0, 0.1 * (ny - 1), ny), M=LEVEL4_M, n=1, seed=3,
                seed2=1003)


def _level4_grid():
    """257 x 65281 = 2^24 + 1 cells: rows 100-119 negative (20 x 65281 cells: whole tiles, a run longer than 64 tiles), the last
    5281 columns of every row zero (a run longer than a tile in every row, and the trailing one).  Only indices and bit-equal
    sums are asked of it (total, cell) and `pre` to its tolerance: no margin is needed (see above on `cell`)."""
    return _level4(257, 65281, "257 x 65281 = 2^24 + 1 cells", 5281)


def _level4_grid_read():
    """257 x 67400 = 17 321 800 cells (4229 tiles), rows 100-119 negative: the cells from 17 043 520 on, 1.6 % of them, lie behind
    the P4 carry, and `total` with them"""
    return _level4(257, 67400, "257 x 67400: 4229 tiles", 0)


_LEVEL_BUILDERS = [("65 x 4033 = 64^3 + 1 cells", _level3_grid), ("65 x 4161: 67 tiles", _level3_grid_read),
                   ("257 x 65281 = 2^24 + 1 cells", _level4_grid), ("257 x 67400: 4229 tiles", _level4_grid_read)]
LEVEL_CASES = [name for name, _ in _LEVEL_BUILDERS]
LEVEL3_CASES, LEVEL4_CASES = LEVEL_CASES[:2], LEVEL_CASES[2:]
_level_built = {}


def level_case(name):
    """the case of that name; the level-3 grids are kept (2 MB each, the CPU and the device test share them), the level-4 grids
    are built anew for whoever asks (134 MB and more: one test each)"""
    if name in _level_built:
        return _level_built[name]
    case = dict(_LEVEL_BUILDERS)[name]()
    if case["data"].size <= 1 << 20:
        _level_built[name] = case
    return case


def restate(case, **kw):
    a = dict(M=case["M"], n=case["n"], seed=case["seed"], seed2=case["seed2"])
    a.update(kw)
    return hm.heatmap_density_numpy(case["data"], case["x"], case["y"], case.get("bw_factor", 0.7), **a)


def margins(case, R):
    """-> (cell, grid, pick): the smallest distance of a cell draw / a pick from an end of its CDF interval relative to the total,
    and of a pre-sample from a grid line or a side of the box relative to the spacing"""
    def cdf_margin(cdf, t, idx):
        lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], -np.inf)
        return float(np.min(np.minimum(cdf[idx] - t, t - lo)) / cdf[-1])
    g = np.inf
    for p, v, s in ((R["pre"][:, 0], case["x"], R["dx"]), (R["pre"][:, 1], case["y"], R["dy"])):
        f = (p - v[0]) / s  # (the sides of the box are the lines 0 and len(v) - 1)
        g = min(g, float(np.min(np.abs(f - np.rint(f)))))
    return cdf_margin(R["cdf"], R["t"], R["cell"].astype(np.int64)), g, cdf_margin(R["wcdf"], R["tw"], R["pick"].astype(np.int64))


def pre_tol(case, R):
    """(M x 2): the bound on |dev - R| of the pre-samples"""
    h = R["h"]
    ny = case["y"].size
    base = np.stack([case["x"][R["cell"] // ny], case["y"][R["cell"] % ny]], axis=1)
    return BM_ATOL * h + EPS * np.abs(R["pre"] - base) + EPS * np.abs(R["pre"])


def d_tol(case, R):
    data = case["data"]
    nx, ny = data.shape
    Gx, Gy = np.abs(np.diff(data, axis=0)).max(), np.abs(np.diff(data, axis=1)).max()
    pt = pre_tol(case, R)
    return Gx * (pt[:, 0] / R["dx"] + 2 * EPS * nx) + Gy * (pt[:, 1] / R["dy"] + 2 * EPS * ny) + 8 * EPS * np.abs(data).max()


def check_stages(case, R, total, cell, pre, d, W, wtotal, pick, points, bw):
    """the device's stages against the restatement R, every figure printed before it is asserted"""
    name = case["name"]
    pt, dt = pre_tol(case, R), d_tol(case, R)
    print(f"{name}: total {total!r} / {R['total']!r}; max |pre - R| / tol = {np.max(np.abs(pre - R['pre']) / pt):.3g}; "
          f"max |d - R| / tol = {np.max(np.abs(d - R['d']) / dt):.3g} (max |d - R| = {np.max(np.abs(d - R['d'])):.3g})")
    assert total == R["total"], name
    np.testing.assert_array_equal(cell, R["cell"], err_msg=name)
    assert np.all(np.abs(pre - R["pre"]) <= pt), name
    assert np.all(np.abs(d - R["d"]) <= dt), name
    Wd = np.exp(np.maximum(-(d - d.min()), -700.0))
    relW, relR = np.max(np.abs(W - Wd) / Wd), np.max(np.abs(W - R["W"]) / R["W"])
    print(f"{name}: max rel |W - exp(-(d - min d))| = {relW:.3g}; against R's W = {relR:.3g}; wtotal {wtotal!r} / {R['wtotal']!r}")
    assert np.all(np.abs(W - Wd) <= W_RTOL * Wd), name
    assert np.all(np.abs(W - R["W"]) <= R["W"] * (W_RTOL + dt + dt.max())), name
    assert wtotal == hm.scan_numpy(W)[-1], name
    np.testing.assert_array_equal(pick, R["pick"], err_msg=name)
    assert np.array_equal(points, pre[pick]), name
    np.testing.assert_array_equal(bw, [R["h"], R["h"]])


# ---- known answers -----------------------------------------------------------------------------------------------------------------
def gaussian_image():
    """test/testHeatmapGridDensity.jl: the pdf of N(0, I) on -10:0.1:10 squared; bw_factor 0.07, N = 1000, 1000 jittered samples"""
    x = np.linspace(-10.0, 10.0, 201)
    img = np.exp(-0.5 * (x[:, None] ** 2 + x[None, :] ** 2)) / (2 * np.pi)
    return img, x, x


GAUSS_SEEDS = [(11, 12), (21, 22), (31, 32)]  # (construction, sample)
GAUSS_MEAN_BAND, GAUSS_COV_BAND = 0.15, 0.4   # the reference's: isapprox(.; atol) is the 2-norm / the Frobenius norm of the difference


def gaussian_bands_ok(pts, what):
    mean, cov = pts.mean(axis=0), np.cov(pts.T, bias=True)  # (fit(MvNormal, .): the maximum-likelihood covariance)
    dm, dc = np.linalg.norm(mean), np.linalg.norm(cov - np.eye(2))
    print(f"{what}: |mean| = {dm:.3f} (band {GAUSS_MEAN_BAND}), |cov - I| = {dc:.3f} (band {GAUSS_COV_BAND})")
    assert dm <= GAUSS_MEAN_BAND and dc <= GAUSS_COV_BAND, what


def cells_field():
    """the 20 x 20 grid with a third of its cells <= 0, and the law of a cell pick: w / total"""
    c = STAGE_CASES[2]
    w = np.where(c["data"] > 0, c["data"], 0.0).reshape(-1)
    return c, w / w.sum()


CELLS_M, CELLS_SEED = 100_000, 5


def bowl():
    """d = 0.5 r^2 / s^2 + c on a 21 x 21 grid, every cell positive: exp(-d) spans e^-8 between the middle and a corner"""
    x = np.linspace(-4.0, 4.0, 21)
    return 0.5 * (x[:, None] ** 2 + x[None, :] ** 2) / 1.5 ** 2 + 1.0, x, x


BOWL_M, BOWL_N, BOWL_SEED = 200, 100_000, 7


# ---- the pass-through path -----------------------------------------------------------------------------------------------------------
def levelset_image():
    """testSpecialEuclidean2Mani.jl:331-340: rand(10, 10) + 5 on (-9:2:9, -9:2:9), level 5.5, sigma 0.1, N = 120"""
    return np.random.default_rng(42).uniform(size=(10, 10)) + 5.0, np.arange(-9.0, 10.0, 2.0), np.arange(-9.0, 10.0, 2.0)


def graph_w_priors(Z, N=N_CTX):
    fg = iif.initfg(iif.SolverParams(N=N))
    iif.addVariable(fg, "x0", iif.SpecialEuclidean2)
    iif.addFactor(fg, ["x0"], iif.PartialPriorPassThrough.fromDensity(iif.SpecialEuclidean2, Z, (1, 2)), label="x0f1")
    return fg


def graph_w_relative(Z, N=N_CTX):
    """testSpecialEuclidean2Mani.jl:456-527 "w Relative" with a real heatmap behind the pass-through prior"""
    fg = graph_w_priors(Z, N)
    iif.addVariable(fg, "x1", iif.SpecialEuclidean2)
    iif.addFactor(fg, ["x1"], iif.ManifoldPrior(np.zeros(3), iif.MvNormal(np.zeros(3), np.diag([0.01, 0.01, 0.01]) ** 2)), label="x1f1")
    iif.addFactor(fg, ["x0", "x1"], iif.ManifoldFactor(iif.MvNormal([1.0, 2.0, np.pi / 4], np.diag([0.01, 0.01, 0.01]) ** 2)), label="x0x1f1")
    return fg

