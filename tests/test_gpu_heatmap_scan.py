"""-m gpu: SCAN and SEARCH of csrc/nbp_heatmap.h by themselves, through nbp_heatmap_scan_eval / nbp_heatmap_search_eval, and the
real heatmap path at the sizes where the sum has a third and a fourth level.

  a  the whole scan, all n elements, bit for bit against `scan_numpy` at every boundary of every level (1 .. 2^26 elements)
  b  the scan against a long-double running sum, within the depth bound of its definition
  c  the search at its edges against `search_numpy` (and numpy's searchsorted where the array is non-decreasing)
  d  create / build / draw on 64^3 + 1 and 2^24 + 1 cells and on 64^3 + 1 pre-samples (heatmap_cases.LEVEL_CASES)
  e  what the two entry points refuse

Why the shapes: a segment is 64 elements, a tile 64 segments, nbp_hm_scan_tiles_kernel forms a P3 carry from 65 tiles on
(n > 64^3) and a P4 carry from 4097 tiles on (n > 2^24); 2^26 is the ceiling (16384 tiles, every wave of that kernel takes four
segments of tile totals).  A carry goes INTO the next segment, so the first sums that contain those two carries are element 64 of
tile 65 and of tile 4161: the lengths "... + 64^2 + 64 + 1" of levels 3 and 4 are the first that read them, and everything longer
does (with `p3[t] + p4[.]` or the final `p2[i] + p3[.]` of that kernel left out, exactly the cases from there on fail, in a and b
alike; at 64^3 + 1 and 2^24 + 1 the carry is computed and nothing reads it).  tests/test_heatmap.py ties `scan_numpy` to a
wave-by-wave walk of that kernel at the same tile counts."""
import ctypes as C
import time

import numpy as np
import pytest

import heatmap_cases as hc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
hm = iif.heatmap
SEG, TILE, GROUP, TOP = 64, 4096, 64 ** 3, 2 ** 24  # segment, tile, 64-tile group, 4096 tiles
MAXN = 1 << 26
ERR_ARG = -1  # NBP_ERR_ARG (include/nbp.h)

LENGTHS = {1: [1, 63, 64, 65],
           2: [4095, 4096, 4097, 4096 + 64 + 1],
           3: [GROUP - 1, GROUP, GROUP + 1, GROUP + 4096, GROUP + 4097, GROUP + 64 ** 2 + 64 + 1, 2 * GROUP + 1],
           4: [TOP, TOP + 1, TOP + GROUP + 64 ** 2 + 64 + 1, MAXN]}
SCAN_CASES = [(n, cls) for lvl in (1, 2, 3) for n in LENGTHS[lvl] for cls in ("i", "ii", "iii")] + \
             [(n, cls) for n in LENGTHS[4] for cls in ("i", "ii")]
BOUND_CASES = [(n, cls) for n, cls in SCAN_CASES if cls != "iii"]
_ids = lambda cases: [f"{n}-{cls}" for n, cls in cases]  # noqa: E731


@pytest.fixture(scope="module")
def be(hip_backend):
    b = hip_backend(hc.N_CTX, 4)
    yield b
    b.close()


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
PERIOD = 1_000_003  # of the 2^26 inputs (a prime: no alignment with segments or tiles); they are laid out without a random stream
_NONPOS = np.array([-0.0, -1.5, 0.0, -0.25, -0.0, -3e-7, -1e12, 0.0])


def nonpositive_runs(n):
    """class (ii): [start, end) of the runs of values <= 0, cut to n -- a short leading run (sums that are exactly +0), whole
    segments, a run that ends on a segment's boundary, one across a tile's boundary, a whole tile, whole tiles up to EXACTLY the
    end of a 64-tile group, one across the first tile boundary of the next group, a whole group (where it fits with an element
    behind it), a whole group up to exactly the end of the first 4096 tiles, and (2^26 only) a run across the boundary at 3 * 4096
    tiles that ends on a group's boundary.  The totals of those segments / tiles / groups are exactly 0 at the upper levels and
    the carries on either side of them equal."""
    runs = [(0, 3)] if n > SEG else []
    runs += [(64, 192), (197, 320), (TILE - 71, TILE + 67), (2 * TILE, 3 * TILE), (GROUP - 3 * TILE - 5 * SEG - 3, GROUP),
             (GROUP + TILE - 67, GROUP + TILE + 2), (TOP - GROUP - TILE - 70, TOP), (3 * TOP - TILE - 3, 3 * TOP + 2 * GROUP)]
    if n > 2 * GROUP:
        runs.append((GROUP, 2 * GROUP))
    return [(a, min(b, n)) for a, b in runs if a < n]


def scan_input(n, cls):
    rng = np.random.default_rng([n, {"i": 1, "ii": 2, "iii": 3}[cls]])
    m = min(n, PERIOD) if n == MAXN else n
    if cls == "i":  # the class of tests/test_heatmap.py
        a = rng.uniform(0, 1, m) * np.exp(rng.normal(0, 3, m))
        a[rng.uniform(size=m) < 0.2] = 0.0
    elif cls == "ii":
        a = rng.uniform(0.1, 2.0, m)
    else:  # later additions are absorbed by 1e12 (half an ulp: 6.1e-5): only the association order decides the bits
        a = rng.uniform(0.5e-6, 1.5e-6, m)
        a[0] = 1e12
    if m < n:
        a = np.resize(a, n)
        if cls == "i":
            a[5 * GROUP - 2 * TILE - 9:5 * GROUP] = 0.0  # the zero run laid in: up to a group's boundary
    if cls == "ii":
        for lo, hi in nonpositive_runs(n):
            a[lo:hi] = np.resize(_NONPOS, hi - lo)
    return a


def weights(a):
    return np.where(a > 0, a, 0.0)


def n_scans(n):
    """how many scans the recursion of the definition makes for n elements"""
    return 1 if n <= SEG else 2 if n <= SEG ** 2 else 3 if n <= SEG ** 3 else 4 if n <= TOP else 5


def where(i):
    return f"index {i}: segment {i // SEG} (element {i % SEG} of it), tile {i // TILE}, 64-tile group {i // GROUP}"


# ---- a. the whole scan at every boundary of every level -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cls", SCAN_CASES, ids=_ids(SCAN_CASES))
def test_whole_scan_is_the_restatement(be, n, cls):
    a = scan_input(n, cls)
    t0 = time.perf_counter()
    s = be.heatmap_scan_eval(a)
    t1 = time.perf_counter()
    a = weights(a)
    want = hm.scan_numpy(a)
    t2 = time.perf_counter()
    print(f"n = {n} ({cls}): {(n + TILE - 1) // TILE} tiles, device call {t1 - t0:.2f} s, restatement {t2 - t1:.2f} s")
    assert s.shape == want.shape == (n,)
    if not np.array_equal(s, want):
        bad = np.flatnonzero(s != want)
        i = int(bad[0])
        pytest.fail(f"n = {n} ({cls}): {bad.size} of {n} sums differ, the first at {where(i)}: device {s[i]!r}, restatement {want[i]!r}; "
                    f"the last at {where(int(bad[-1]))}")
    assert not np.signbit(s).any()  # negatives and -0.0 count as +0.0: no sum is -0.0
    if cls == "ii" and n > SEG:
        assert s[0] == 0.0 and s[2] == 0.0 and s[3] > 0.0  # (the leading run: sums that are exactly 0)


# ---- b. the definition against a high-precision sum ----------------------------------------------------------------------------------------
def long_double_cumsum(w, chunk=1 << 22):
    """np.cumsum(w.astype(np.longdouble)), the same additions in the same order, handed out in chunks (2^26 long doubles are 1 GB)"""
    carry = np.longdouble(0)
    for lo in range(0, w.size, chunk):
        e = np.cumsum(np.concatenate([[carry], w[lo:lo + chunk].astype(np.longdouble)]))[1:]
        carry = e[-1]
        yield lo, e


@pytest.mark.parametrize("n,cls", BOUND_CASES, ids=_ids(BOUND_CASES))
def test_scan_is_within_the_depth_bound_of_its_definition(be, n, cls):
    """every partial sum is a tree over non-negative terms, at most 6 additions deep per level plus one carry addition per
    level: |s[i] - e[i]| <= 7 L 2^-53 e[i], L = the scans the recursion makes for n -- from the definition, not from the kernels"""
    assert np.finfo(np.longdouble).nmant >= 63
    a = scan_input(n, cls)
    s = be.heatmap_scan_eval(a)
    w = weights(a)
    L = n_scans(n)
    worst, at = 0.0, -1
    for lo, e in long_double_cumsum(w):
        err = s[lo:lo + e.size] - e  # (in long double)
        zero = e == 0
        assert np.all(err[zero] == 0), f"n = {n} ({cls}): a sum of zeros is not 0 in the chunk from {where(lo)}"
        # the ratio to the bound in double (quick, and within 1e-15 of itself) ...
        r = np.abs(err.astype(np.float64)) / np.where(zero, 1.0, 7 * L * 2.0 ** -53 * e.astype(np.float64))
        if r.max() > 0.99:  # ... and where that could decide, in long double
            r = np.abs(err) / np.where(zero, 1, 7 * L * np.longdouble(2.0) ** -53 * e)
        k = int(np.argmax(r))
        if float(r[k]) > worst:
            worst, at = float(r[k]), lo + k
    print(f"n = {n} ({cls}): L = {L}, bound {7 * L} * 2^-53 relative; largest |s - e| / bound = {worst:.3f}" + (f" at {where(at)}" if at >= 0 else ""))
    assert worst <= 1.0, f"n = {n} ({cls}): |s - e| = {worst:.3f} x the bound at {where(at)}"


# ---- c. the search at its edges --------------------------------------------------------------------------------------------------------------
def edge_probes(cdf, seed):
    """cdf[i] and its two neighbours among the doubles for every i within 2 of every segment end (tile ends and group ends are
    among them) and of the last element; 0, -1, cdf[n-1], 2 cdf[n-1], NaN; the value of every plateau and the double below it;
    200 000 uniform probes over [0, cdf[n-1])"""
    n = cdf.size
    ends = np.concatenate([np.arange(SEG - 1, n, SEG), [n - 1]])
    idx = np.unique(np.clip(ends[:, None] + np.arange(-2, 3)[None, :], 0, n - 1))
    v = cdf[idx]
    same = cdf[1:] == cdf[:-1]
    start = np.flatnonzero(same & ~np.concatenate([[False], same[:-1]]))  # the first element of every plateau
    p = cdf[start]
    fixed = np.array([0.0, -1.0, cdf[n - 1], 2.0 * cdf[n - 1], np.nan])
    u = np.random.default_rng([n, seed]).uniform(0.0, 1.0, 200_000) * cdf[n - 1]
    return np.concatenate([fixed, v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), p, np.nextafter(p, -np.inf), u]), start.size


def check_search(be, cdf, what, seed=0):
    n = cdf.size
    t, plateaus = edge_probes(cdf, seed)
    t0 = time.perf_counter()
    got = be.heatmap_search_eval(cdf, t)
    want = hm.search_numpy(cdf, t)
    monotone = bool(np.all(cdf[1:] >= cdf[:-1]))
    print(f"{what}: n = {n}, {(n + TILE - 1) // TILE} tiles, {t.size} probes, {plateaus} plateaus, non-decreasing: {monotone}, "
          f"{time.perf_counter() - t0:.2f} s")
    assert got.dtype == np.int32 and got.shape == t.shape
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: {int(np.sum(got != want))} of {t.size} probes differ, the first: t = {t[k]!r} -> device {got[k]} "
                    f"({where(int(got[k]))}), restatement {want[k]} ({where(int(want[k]))})")
    assert want[3] == n - 1 and want[4] == n - 1  # 2 cdf[n-1] and NaN (t < cdf[mid] is false for it: right at every probe)
    if monotone:
        assert np.array_equal(want, np.minimum(np.searchsorted(cdf, t, side="right"), n - 1)), what
        assert want[2] == n - 1  # cdf[n-1] itself: no element with t < cdf is left
    return monotone


@pytest.mark.parametrize("n", [4097, GROUP + 4097, TOP + 1])
def test_search_on_the_device_s_own_scan(be, n):
    """the scan of class (ii): plateaus across segment, tile and group boundaries (a plateau that is not flat to the last bit -- the
    sums of one segment associate differently from element to element -- is the non-monotone case, decided probe by probe)"""
    a = scan_input(n, "ii")
    cdf = be.heatmap_scan_eval(a)
    for b in [e for e in (SEG, TILE, GROUP, TOP) if e < n]:
        assert not a[b - 1] > 0 or not a[b] > 0  # a run of weight 0 reaches the boundary from one side or crosses it
        print(f"n = {n}: at the boundary {b}: cdf[b-2 .. b] - cdf[b-1] = {(cdf[b - 2:b + 1] - cdf[b - 1]).tolist()}")
    if not check_search(be, cdf, f"scan of class (ii), n = {n}") and n <= 2 * GROUP:
        # the same plateaus made flat: non-decreasing, so numpy's searchsorted has its say at this size too
        assert check_search(be, np.maximum.accumulate(cdf), f"running maximum of that scan, n = {n}", seed=1)


def dipped(n, seed):
    """a running sum with the element at every tile end (but the last element) one ulp BELOW its predecessor, and one such dip
    in the middle of a tile: nothing but the probe-by-probe rule says where a search ends"""
    cdf = np.cumsum(np.random.default_rng([n, seed]).uniform(0.1, 2.0, n))
    dips = [e for e in list(range(TILE - 1, n - 1, TILE)) + [2 * TILE + 1000, n // 2] if 1 <= e < n - 1]
    for e in dips:
        cdf[e] = np.nextafter(cdf[e - 1], -np.inf)
    return cdf, len(dips)


def test_search_on_a_non_monotone_array(be):
    cdf, dips = dipped(GROUP + 4097, 1)
    assert dips == 65 + 2 and not check_search(be, cdf, "dips at the tile ends")  # (66 tiles: 0 .. 64 end before the last element)


@pytest.mark.parametrize("n", [1, 2, 4096, 4097])
def test_search_on_one_and_two_tiles(be, n):
    """the tile loop with nothing to bisect (one tile) and with one probe (two)"""
    w = np.random.default_rng(n).uniform(0.1, 2.0, n)
    if n >= TILE:
        w[n // 3:n // 3 + 70] = 0.0  # a plateau across a segment end
    if n == 4097:
        w[4090:] = 0.0  # a plateau across the tile end, up to the last element
    assert check_search(be, np.cumsum(w), f"running sum, n = {n}")
    if n > 2:
        assert not check_search(be, dipped(n, 2)[0], f"dipped running sum, n = {n}")


# ---- d. the real path at the third and the fourth level ------------------------------------------------------------------------------------------
def run(be, case):
    """create, build, draw, destroy -> (total, cell, pre, d, W, wtotal, pick, points, bw)"""
    h = be.heatmap_create(case["data"], case["x"], case["y"], case.get("bw_factor", 0.7))
    try:
        cell, pre, d, W = be.heatmap_build(h, case["M"], case["seed"])
        bw, total, wtotal, Mi = be.heatmap_info(h)
        assert Mi == len(cell)
        pick, pts, bw2 = be.heatmap_draw(h, case["n"], case["seed2"])
        assert np.array_equal(bw, bw2)
        return total, cell, pre, d, W, wtotal, pick, pts, bw
    finally:
        be.heatmap_destroy(h)


@pytest.mark.parametrize("name", hc.LEVEL3_CASES)
def test_third_level_grid_stage_by_stage(be, name):
    """65 x 4033 = 64^3 + 1 cells (the first length whose tile totals have a P3 carry) and 65 x 4161 (67 tiles: 1.5 % of the picks
    lie behind it), M = 100 000, every stage"""
    case = hc.level_case(name)
    hc.check_stages(case, hc.restate(case), *run(be, case))


@pytest.mark.parametrize("name", hc.LEVEL4_CASES)
def test_fourth_level_grid(be, name):
    """257 x 65281 = 2^24 + 1 cells (134 MB; rows 100-119 negative, the last 5281 columns of every row zero: 4097 tiles, the
    first length with a P4 carry) and 257 x 67400 (4229 tiles: `total` and 1.6 % of the picks lie behind it), M = 100 000"""
    case = hc.level_case(name)
    data, flat = case["data"], case["data"].reshape(-1)
    assert flat.size >= hc.LEVEL4_CELLS and np.all(data[100:120] <= 0)
    if flat.size == hc.LEVEL4_CELLS:
        assert not data[:, -5281:].any()
    t0 = time.perf_counter()
    R = hc.restate(case)
    t1 = time.perf_counter()
    h = be.heatmap_create(data, case["x"], case["y"])
    try:
        bw, total, wtotal, Mi = be.heatmap_info(h)
        assert Mi == 0 and wtotal == 0.0 and np.array_equal(bw, [R["h"], R["h"]])
        cell, pre, d, W = be.heatmap_build(h, case["M"], case["seed"])
        bw, total2, wtotal, Mi = be.heatmap_info(h)
    finally:
        be.heatmap_destroy(h)
    print(f"{name}: restatement {t1 - t0:.2f} s, device {time.perf_counter() - t1:.2f} s; total {total!r} / {R['total']!r}; "
          f"max |pre - R| / tol = {np.max(np.abs(pre - R['pre']) / hc.pre_tol(case, R)):.3g}; cells picked {cell.min()} .. {cell.max()}, "
          f"{int(np.sum(R['cell'] >= hc.LEVEL4_READ))} behind the P4 carry")
    assert total == R["total"] and total2 == total
    np.testing.assert_array_equal(cell, R["cell"])  # (cdf and the draws are the same bits on both sides: equal whatever the margin)
    assert np.all(flat[cell] > 0)
    assert np.all(np.abs(pre - R["pre"]) <= hc.pre_tol(case, R))
    assert Mi == case["M"] and np.array_equal(bw, [R["h"], R["h"]]) and wtotal == hm.scan_numpy(W)[-1]
    if flat.size > hc.LEVEL4_READ:
        assert np.sum(R["cell"] >= hc.LEVEL4_READ) > 1000


@pytest.mark.parametrize("M", hc.PRE_LEVEL3_MS)
def test_third_level_of_the_pre_samples(be, M):
    """the 20 x 20 grid with M = 64^3 + 1 pre-samples (65 tiles of weights) and M = 64^3 + 2 * 4096 + 1 (67 tiles: 1.5 % of the picks
    lie behind the P3 carry): the second sum, over W, and 200 000 draws bisecting its tiles"""
    case, n = hc.STAGE_CASES[2], hc.PRE_LEVEL3_N
    R = hc.restate(case, M=M, n=1)
    h = be.heatmap_create(case["data"], case["x"], case["y"])
    try:
        cell, pre, d, W = be.heatmap_build(h, M, case["seed"])
        _, total, wtotal, Mi = be.heatmap_info(h)
        pick, pts, _ = be.heatmap_draw(h, n, case["seed2"])
    finally:
        be.heatmap_destroy(h)
    assert Mi == M and total == R["total"]
    np.testing.assert_array_equal(cell, R["cell"])
    wcdf = hm.scan_numpy(W)  # (the device's own W: the same sums)
    assert wtotal == wcdf[-1]
    assert np.array_equal(be.heatmap_scan_eval(W), wcdf)
    ua, _ = hm.uniform_pairs(case["seed2"], np.arange(n), hm.PURP_HMPICK, 0)
    want = hm.search_numpy(wcdf, ua * wtotal)
    behind = int(np.sum(want >= hc.LEVEL3_READ))
    print(f"M = {M}: wtotal {wtotal!r}; picks {pick.min()} .. {pick.max()}, {behind} of {n} behind the P3 carry")
    assert np.array_equal(pick, want)
    assert np.array_equal(pts, pre[pick])
    assert behind > 1000 or M <= hc.LEVEL3_READ


# ---- e. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_two_entry_points(be):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a, out, idx = np.arange(1.0, 9.0), np.zeros(8), np.zeros(8, dtype=np.int32)
    pa, po, pi = a.ctypes.data_as(dp), out.ctypes.data_as(dp), idx.ctypes.data_as(ip)
    scan, search, ctx = be.lib.nbp_heatmap_scan_eval, be.lib.nbp_heatmap_search_eval, be._ctx
    for n in (0, -1, MAXN + 1):  # (the sizes are looked at before the buffers: 8 doubles behind the pointers are enough)
        assert scan(ctx, pa, n, po) == abi.ERR_INVALID and b"2^26" in be.lib.nbp_last_error(), n
        assert search(ctx, pa, n, pa, 8, pi) == abi.ERR_INVALID, n
        assert search(ctx, pa, 8, pa, n, pi) == abi.ERR_INVALID, n
    assert scan(ctx, None, 8, po) == ERR_ARG and scan(ctx, pa, 8, None) == ERR_ARG and scan(None, pa, 8, po) == ERR_ARG
    assert search(ctx, None, 8, pa, 8, pi) == ERR_ARG and search(ctx, pa, 8, None, 8, pi) == ERR_ARG
    assert search(ctx, pa, 8, pa, 8, None) == ERR_ARG and search(None, pa, 8, pa, 8, pi) == ERR_ARG
    assert not out.any() and not idx.any()  # nothing was written
    with pytest.raises(iif.NbpError, match=f"status {abi.ERR_INVALID}:"):
        be.heatmap_scan_eval(np.zeros(0))
    # the context stays usable
    assert np.array_equal(be.heatmap_scan_eval([1.0, -2.0, 2.0, -0.0, 3.0]), [1.0, 1.0, 3.0, 3.0, 6.0])
    assert be.heatmap_search_eval([1.0, 1.0, 3.0, 3.0, 6.0], [0.5, 1.0, 2.9, 3.0, 6.0, 7.0]).tolist() == [0, 2, 2, 4, 4, 4]
