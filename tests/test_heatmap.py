"""Heatmap densities on the CPU: `heatmap_density_numpy`, the host restatement of csrc/nbp_heatmap.h, alone -- its pieces against
their definitions, the conditions under which tests/test_gpu_heatmap.py and tests/test_gpu_heatmap_scan.py may ask for equal
indices, and the known answers of tests/heatmap_cases.py.  Nothing here runs libnbp."""
import math
import types

import numpy as np
import pytest

import heatmap_cases as hc
import sampling_cases as sc
from parity_utils import iif

hm = iif.heatmap


def test_streams_are_the_python_philox():
    for seed in (1, 0xDEADBEEF00000001, 2 ** 64 - 1):
        for purpose, k in ((hm.PURP_HMCELL, 0), (hm.PURP_HMNOISE, 1), (hm.PURP_HMPICK, 0)):
            ua, ub = hm.uniform_pairs(seed, np.arange(40), purpose, k)
            for n in range(40):
                assert (ua[n], ub[n]) == sc.uniform_pair(seed, n, purpose, k)
    assert (hm.PURP_HMCELL, hm.PURP_HMNOISE, hm.PURP_HMPICK) == (16, 17, 18)  # the next free numbers after PURP_PINDEX = 15


def _ks(v):
    v = v.copy()
    for o in (1, 2, 4, 8, 16, 32):
        v = np.where(np.arange(64) >= o, v + np.concatenate([np.zeros(o), v[:-o]]), v)
    return v


def tiles_kernel(t2):
    """nbp_hm_scan_tiles_kernel walked wave by wave: T2 -> l2 (kept in p2) and T3; T3 -> l3 and T4; P4 = l4; P3 = l3 + P4[.];
    P2 = l2 + P3[.] -- m <= 2^14 tile totals -> P2 = scan(T2), the carries as the kernel forms them"""
    m = t2.size
    assert m <= 1 << 14
    p2, t3, p3, t4 = np.zeros(m), np.zeros(256), np.zeros(256), np.zeros(4)
    nseg2 = -(-m // 64)
    nseg3 = -(-nseg2 // 64)
    for src, cnt_all, dst, tot in ((t2, m, p2, t3), (t3, nseg2, p3, t4)):
        for s in range(-(-cnt_all // 64)):
            cnt = min(64, cnt_all - s * 64)
            v = np.zeros(64)
            v[:cnt] = src[s * 64:s * 64 + cnt]
            r = _ks(v)
            dst[s * 64:s * 64 + cnt], tot[s] = r[:cnt], r[cnt - 1]
    v = np.zeros(64)
    v[:nseg3] = t4[:nseg3]
    p4 = _ks(v)
    for t in range(64, nseg2):
        p3[t] = p3[t] + p4[t // 64 - 1]
    for i in range(64, m):
        p2[i] = p2[i] + p3[i // 64 - 1]
    return p2


def scan_by_tiles(a):
    """the three scan kernels of csrc/nbp_heatmap.h walked tile by tile, wave by wave (zero-padded segments, the carries as the
    kernels form them): what the recursive definition must agree with bit for bit"""
    n = a.size
    tiles = -(-n // 4096)

    def segments(b):
        l, t1 = np.zeros((64, 64)), np.zeros(64)
        for seg in range(64):
            i0 = b * 4096 + seg * 64
            cnt = min(64, n - i0)
            if cnt > 0:
                v = np.zeros(64)
                v[:cnt] = a[i0:i0 + cnt]
                l[seg] = _ks(v)
                t1[seg] = l[seg][cnt - 1]
        return l, t1
    seg_of = [segments(b) for b in range(tiles)]
    t2 = np.array([_ks(t1)[min(64, -(-(n - b * 4096) // 64)) - 1] for b, (_, t1) in enumerate(seg_of)])
    p2 = tiles_kernel(t2)
    out = np.zeros(n)
    for b, (l, t1) in enumerate(seg_of):
        l1 = _ks(t1)
        for seg in range(64):
            i0 = b * 4096 + seg * 64
            cnt = min(64, n - i0)
            if cnt <= 0:
                break
            if seg > 0:
                carry = l1[seg - 1] + p2[b - 1] if b > 0 else l1[seg - 1]
            else:
                carry = None if b == 0 else t2[0] if b == 1 else t2[b - 1] + p2[b - 2]
            out[i0:i0 + cnt] = l[seg][:cnt] if carry is None else l[seg][:cnt] + carry
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 65, 300 * 257, 64 ** 3 + 1, 64 ** 3 + 64 ** 2 + 64 + 1])
def test_scan_is_the_documented_order(n):
    rng = np.random.default_rng(n)
    a = rng.uniform(0, 1, n) * np.exp(rng.normal(0, 3, n))
    a[rng.uniform(size=n) < 0.2] = 0.0
    s = hm.scan_numpy(a)
    assert np.array_equal(s, scan_by_tiles(a))
    # every partial sum is a tree of depth <= 6 per level over non-negative terms: within (6 levels') eps of the exact sum
    for i in sorted({0, n // 3, n - 1}):
        exact = math.fsum(a[:i + 1])
        assert abs(s[i] - exact) <= 30 * 2.0 ** -53 * exact
    if n <= 64:  # one segment: the plain Kogge-Stone sums
        assert np.array_equal(s, _ks(np.concatenate([a, np.zeros(64 - n)]))[:n])


@pytest.mark.parametrize("m", [64, 65, 4096, 4097, 16384])
def test_tiles_kernel_walk_is_the_scan_of_the_tile_totals(m):
    """the second kernel alone, up to the 2^14 tile totals of 2^26 elements (scan_by_tiles takes too long there): scan_numpy's
    third and fourth level are the kernel's own carry order -- m = 64: no carry; 65: the first P3 carry; 4096: nseg3 = 1 still;
    4097: the first P4 carry; 16384: four segments at the fourth level.  tests/test_gpu_heatmap_scan.py then holds the device to
    scan_numpy at the lengths these m belong to."""
    rng = np.random.default_rng(m)
    t2 = rng.uniform(0, 1, m) * np.exp(rng.normal(0, 3, m))
    t2[rng.uniform(size=m) < 0.2] = 0.0
    assert np.array_equal(tiles_kernel(t2), hm.scan_numpy(t2))


def test_search_is_the_first_element_above():
    rng = np.random.default_rng(3)
    for n in (1, 2, 64, 4096, 4097, 20000):
        cdf = np.cumsum(rng.uniform(0, 1, n) * (rng.uniform(size=n) < 0.7))
        cdf[-1] += 1.0
        t = np.concatenate([rng.uniform(0, cdf[-1], 2000), cdf[rng.integers(0, n, 200)], [0.0]])
        t = t[t < cdf[-1]]
        assert np.array_equal(hm.search_numpy(cdf, t), np.searchsorted(cdf, t, side="right"))
        assert hm.search_numpy(cdf, np.array([cdf[-1], 2 * cdf[-1]])).tolist() == [n - 1, n - 1]  # where rounding leaves none: the last


def test_bilinear_formula():
    x, y = np.linspace(100.0, 138.0, 20), np.linspace(-3.0, 5.0, 9)
    dx, dy = (x[-1] - x[0]) / 19, (y[-1] - y[0]) / 8
    plane = 2.0 + 0.25 * x[:, None] - 1.5 * y[None, :]
    rng = np.random.default_rng(4)
    px, py = rng.uniform(x[0], x[-1], 1000), rng.uniform(y[0], y[-1], 1000)
    px[:4], py[:4] = [x[0], x[-1], x[0], x[-1]], [y[0], y[0], y[-1], y[-1]]  # the corners: the clamp to nx - 2 / ny - 2
    got = hm.bilinear_numpy(plane, x[0], y[0], dx, dy, px, py)
    np.testing.assert_allclose(got, 2.0 + 0.25 * px - 1.5 * py, rtol=0, atol=1e-12)  # bilinear interpolation reproduces a plane
    np.testing.assert_allclose(got[:4], [plane[0, 0], plane[-1, 0], plane[0, -1], plane[-1, -1]], rtol=0, atol=1e-12)
    nodes = hm.bilinear_numpy(plane, x[0], y[0], dx, dy, np.repeat(x, 9), np.tile(y, 20))
    np.testing.assert_allclose(nodes, plane.reshape(-1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", hc.STAGE_CASES, ids=[c["name"] for c in hc.STAGE_CASES])
def test_stage_cases_are_decidable_and_consistent(case):
    """the margins that let the device test ask for equal indices, and the restatement's own stages against their definitions"""
    R = hc.restate(case)
    m = hc.margins(case, R)
    print(case["name"], "margins (cell, grid, pick):", m)
    assert min(m) > hc.MARGIN, m
    data, x, y = case["data"], case["x"], case["y"]
    flat = data.reshape(-1)
    dx, dy = (x[-1] - x[0]) / (x.size - 1), (y[-1] - y[0]) / (y.size - 1)
    assert R["h"] == 0.7 * 0.5 * (dx + dy) and R["total"] == R["cdf"][-1] > 0
    assert np.all(flat[R["cell"]] > 0)
    # the cell IS the first one whose cdf exceeds the draw (the sums are monotone to the last bit at these draws)
    assert np.array_equal(R["cell"], np.searchsorted(R["cdf"], R["t"], side="right"))
    i, j = R["cell"] // y.size, R["cell"] % y.size
    assert np.abs((R["pre"][:, 0] - x[i]) / R["h"]).max() < 6 and np.abs((R["pre"][:, 1] - y[j]) / R["h"]).max() < 6
    assert np.all(R["d"][~R["inside"]] == 0.0)
    if R["inside"].any():
        assert R["d"][R["inside"]].min() >= data.min() - 1e-9 and R["d"][R["inside"]].max() <= data.max() + 1e-9
    assert R["W"].max() == 1.0 and R["W"].min() > 0 and np.all(np.isfinite(R["W"]))
    np.testing.assert_allclose(R["W"], np.exp(np.maximum(-(R["d"] - R["d"].min()), -700.0)), rtol=1e-15)  # (the clamp of exp_nonpos)
    assert np.array_equal(R["points"], R["pre"][R["pick"]]) and R["points"].shape == (case["n"], 2)
    J = hc.restate(case, jitter=1)
    assert np.array_equal(J["pick"], R["pick"]) and np.abs((J["points"] - R["points"]) / R["h"]).max() < 6
    assert not np.array_equal(J["points"], R["points"])


@pytest.mark.parametrize("name", hc.LEVEL3_CASES)
def test_level3_grids_are_decidable_where_a_criterion_needs_it(name):
    """64^3 + 1 cells and 67 tiles of cells, M = 100 000: the grid and the pick margins (what `d` and `pick` of check_stages need)
    exceed MARGIN on the seed chosen; the cell margin is printed -- no criterion needs it and no seed has it (heatmap_cases)"""
    case = hc.level_case(name)
    assert case["data"].size >= hc.LEVEL3_CELLS and 0.05 < np.mean(~(case["data"] > 0)) < 0.15
    R = hc.restate(case)
    cell_m, grid_m, pick_m = hc.margins(case, R)
    print(name, "margins (cell, grid, pick):", (cell_m, grid_m, pick_m))
    assert min(grid_m, pick_m) > hc.MARGIN, (grid_m, pick_m)
    flat = case["data"].reshape(-1)
    assert np.all(flat[R["cell"]] > 0) and R["total"] == R["cdf"][-1] > 0
    assert np.array_equal(R["points"], R["pre"][R["pick"]]) and R["points"].shape == (case["n"], 2)
    if case["data"].size > hc.LEVEL3_READ:
        assert np.sum(R["cell"] >= hc.LEVEL3_READ) > 1000  # pre-samples do land behind the P3 carry


def test_offset_field_keeps_its_weights():
    """an elevation in metres: the reference's exp(-d) is 0 for every pre-sample (0 / 0 after normalisation); exp(-(d - dmin)) is not"""
    case = next(c for c in hc.STAGE_CASES if "800" in c["name"])
    R = hc.restate(case)
    assert np.all(np.exp(-R["d"][R["inside"]]) == 0.0) and R["wtotal"] >= 1.0 and np.all(R["W"] > 0)


def test_refusals():
    x = np.linspace(0.0, 1.0, 5)
    ok = np.ones((5, 5))
    hm.check_grid(ok, x, x, 0.7)
    bad = [(ok, x ** 2 + x, x), (ok, x[::-1].copy(), x), (ok, x, np.array([0.0, 0.25, 0.5, 0.75, 1.0 + 1e-8])),
           (np.ones((1, 5)), x[:1], x), (np.ones((5, 1)), x, x[:1]), (np.where(np.eye(5) > 0, np.nan, 1.0), x, x),
           (np.where(np.eye(5) > 0, np.inf, 1.0), x, x), (-ok, x, x), (np.zeros((5, 5)), x, x), (np.ones((4, 5)), x, x)]
    for data, xx, yy in bad:
        with pytest.raises(ValueError):
            hm.check_grid(data, xx, yy, 0.7)
    for bwf in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            hm.check_grid(ok, x, x, bwf)
    hm.check_grid(ok, x, np.array([0.0, 0.25, 0.5, 0.75, 1.0 + 1e-10]), 0.7)  # uniform to 1e-9 of the spacing
    with pytest.raises(ValueError):
        hm.heatmap_density_numpy(ok, x, x, M=0)


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seeds", hc.GAUSS_SEEDS)
def test_gaussian_image_within_the_reference_bands(seeds):
    img, x, y = hc.gaussian_image()
    R = hm.heatmap_density_numpy(img, x, y, 0.07, M=1000, n=1000, seed=seeds[0], seed2=seeds[1], jitter=1)
    hc.gaussian_bands_ok(R["points"], f"restatement, seeds {seeds}")


def test_cell_picks_follow_the_field():
    case, p = hc.cells_field()
    R = hc.restate(case, M=hc.CELLS_M, n=1, seed=hc.CELLS_SEED)
    sc.chi2_ok(np.bincount(R["cell"], minlength=p.size), p, "cell picks on the 20 x 20 grid")  # (a cell of weight 0: never, exactly)


def test_picks_concentrate_like_exp_minus_d_and_the_check_has_power():
    d, x, y = hc.bowl()
    R = hm.heatmap_density_numpy(d, x, y, M=hc.BOWL_M, n=hc.BOWL_N, seed=hc.BOWL_SEED, seed2=hc.BOWL_SEED + 1)
    counts = np.bincount(R["pick"], minlength=hc.BOWL_M)
    sc.chi2_ok(counts, R["W"] / R["W"].sum(), "picks on the bowl")
    assert R["W"].min() < 0.05  # the weights do differ: the bowl spans e^-8
    with pytest.raises(AssertionError):
        sc.chi2_ok(counts, np.full(hc.BOWL_M, 1.0 / hc.BOWL_M), "picks on the bowl against EQUAL weights")


def test_jitter_is_standard_normal_in_bandwidths():
    d, x, y = hc.bowl()
    R = hm.heatmap_density_numpy(d, x, y, M=hc.BOWL_M, n=hc.BOWL_N, seed=hc.BOWL_SEED, seed2=hc.BOWL_SEED + 1, jitter=1)
    sc.gaussian_ok((R["points"] - R["pre"][R["pick"]]) / R["h"], [0.0, 0.0], np.eye(2), "jitter of the restatement")


# ---- the mirror without a device -----------------------------------------------------------------------------------------------------
def test_from_density_reads_points_and_bandwidth():
    pts, bw = np.arange(12.0).reshape(6, 2), np.array([0.7, 0.7])
    Z = types.SimpleNamespace(points=pts, bw=bw)
    for z in (Z, types.SimpleNamespace(heatmap=Z, level=5.5, sigma=0.1)):
        f = iif.PartialPriorPassThrough.fromDensity(iif.SpecialEuclidean2, z, (1, 2))
        assert isinstance(f, iif.PartialPriorPassThrough) and f.partial == (1, 2)
        assert np.array_equal(f.points, pts) and np.array_equal(f.bw, bw)
    for name in ("HeatmapGridDensity", "LevelSetGridNormal", "heatmap_density_numpy", "sample"):
        assert hasattr(iif, name)


def test_no_numpy_fallback_behind_the_classes():
    """backend=None means libnbp: without a device the constructor raises, it does not quietly restate on the host"""
    import torch
    img, x, y = hc.levelset_image()
    if torch.cuda.is_available():
        assert iif.LevelSetGridNormal(img, (x, y), 5.5, 0.1, N=120).heatmap.points.shape == (120, 2)
    else:
        with pytest.raises(iif.NbpError):
            iif.LevelSetGridNormal(img, (x, y), 5.5, 0.1, N=120)
