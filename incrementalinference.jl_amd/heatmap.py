"""Heatmap priors: a scalar field on a regular x-y grid as a samplable density, built on the device.

  HeatmapGridDensity(data, domain, ...)     the reference's HeatmapGridDensity (ext/HeatmapSampler.jl:162-210): an elevation model or
                                            a correlation surface turned into the density a PartialPriorPassThrough hands to
                                            inference as it is (`PartialPriorPassThrough.fromDensity`)
  LevelSetGridNormal(data, domain, l, s)    its legacy constructor (:229-242), with the heatmap in `.heatmap`
  sample(hgd, n, seed)                      AMP.sample(hgd, n) (:113): kernel pick + h * randn
  heatmap_density_numpy(...)                the host restatement of every stage -- for tests and readers, never a fallback

The definitions ("Heatmap densities"; csrc/nbp_heatmap.h is the device's copy), for data[i, j] at (x[i], y[j]) on a
uniform grid with spacings dx, dy:

  h       bw_factor * 0.5 * (dx + dy), both coordinates.
  cells   w_c = data_c where 0 < data_c, else 0, c = i * ny + j; cdf = scan(w) (`scan_numpy`: the fixed-order prefix sum);
          total = cdf[-1].
  pre     m = 0 .. M-1: (ua, _) = uniform_pair(seed, m, PURP_HMCELL, 0); c = search(cdf, ua * total) (`search_numpy`), moved on to
          the next cell with w > 0 should w_c be 0 (the last such cell where none follows); (n0, n1) = normal_pair(seed, m,
          PURP_HMNOISE, 0); p_m = (x[i] + h * n0, y[j] + h * n1).
  d       the bilinear interpolation of data at p_m (`bilinear_numpy`) inside [x[0], x[-1]] x [y[0], y[-1]], else 0.
  W       W_m = exp(max(-(d_m - dmin), -700)), dmin = min_m d_m; wcdf = scan(W); wtotal = wcdf[-1].
  draw    k = 0 .. n-1: (ua, _) = uniform_pair(seed2, k, PURP_HMPICK, 0); pick = search(wcdf, ua * wtotal); point = pre[pick], with
          jitter + h * normal_pair(seed2, k, PURP_HMNOISE, 1); bandwidth (h, h).

Where this departs from the reference: the grid is checked, not assumed; "outside" is the grid's own box (the reference
tests max(domain) < abs(u), the same box only for a domain symmetric about 0); the weights are taken relative to their largest (equal
after normalisation, and finite for a field in metres); the density is n unweighted points resampled from the M weighted
pre-samples, because a belief here is unweighted and a slot holds at most N points.  `hint_callback` is kept and never called (the
reference marks it "NOT ACTIVE YET")."""
import numpy as np

from . import abi
from .beliefquery import _backend

PURP_HMCELL, PURP_HMNOISE, PURP_HMPICK = 16, 17, 18  # csrc/nbp_heatmap.h (the next free purposes after PURP_PINDEX = 15)
NBP_TAG = 0x4E4250
SEG, TILE = 64, 4096
MAX_CELLS = abi.HM_MAX_CELLS
_M32 = np.uint64(0xFFFFFFFF)


# ---- the random streams (DESIGN.md "RNG"): Philox4x32-10, counter (n, purpose, k, NBP_TAG), key = the seed ------------------------
def uniform_pairs(seed, n, purpose, k):
    """(ua, ub) of blocks (n[i], purpose, k) of the stream keyed `seed`, n an array of counters below 2^32"""
    c0 = np.asarray(n, dtype=np.uint64)
    c1, c2, c3 = np.full_like(c0, purpose), np.full_like(c0, k), np.full_like(c0, NBP_TAG)
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    s11 = np.uint64(11)
    ua = ((((c1 << s32) | c0) >> s11).astype(np.float64) + 0.5) * 2.0 ** -53
    ub = ((((c3 << s32) | c2) >> s11).astype(np.float64) + 0.5) * 2.0 ** -53
    return ua, ub


def normal_pairs(seed, n, purpose, k):
    """Box-Muller on the pair (include/nbp_math.h nbpm_box_muller, here through numpy's log, cos and sin)"""
    ua, ub = uniform_pairs(seed, n, purpose, k)
    r, a = np.sqrt(-2.0 * np.log(ua)), (2.0 * np.pi) * ub
    return r * np.cos(a), r * np.sin(a)


# ---- the fixed-order prefix sum and the search --------------------------------------------------------------------------------------
def _segments(a):
    """the Kogge-Stone steps within segments of 64: l[i] += l[i - o] for every i >= o of its segment, o = 1, 2, .. 32"""
    n = a.size
    l = np.zeros(-(-n // SEG) * SEG)  # (the padding of a short last segment is never read by an element of the segment)
    l[:n] = a
    l = l.reshape(-1, SEG)
    for o in (1, 2, 4, 8, 16, 32):
        l[:, o:] = l[:, o:] + l[:, :-o]
    return l.reshape(-1)[:n]


def scan_numpy(a):
    """the inclusive prefix sum of csrc/nbp_heatmap.h: its order is a function of len(a) alone, one rounding per addition"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    n, l = a.size, _segments(a)
    if n <= SEG:
        return l
    last = np.minimum(np.arange(1, -(-n // SEG) + 1) * SEG, n) - 1
    P = scan_numpy(l[last])
    out = l.copy()
    out[SEG:] = l[SEG:] + np.repeat(P[:-1], SEG)[:n - SEG]
    return out


def _bisect(cdf, t, lo, hi, probe):
    lo, hi = lo.copy(), hi.copy()
    while True:
        act = lo < hi
        if not act.any():
            return hi
        mid = (lo + hi) >> 1
        left = t < cdf[probe(mid)]
        hi = np.where(act & left, mid, hi)
        lo = np.where(act & ~left, mid + 1, lo)


def search_numpy(cdf, t):
    """the two binary searches of csrc/nbp_heatmap.h, probe for probe: over the tiles of 4096 (the tile's last element), then within"""
    n = cdf.size
    t = np.asarray(t, dtype=np.float64)
    z = np.zeros(t.shape, dtype=np.int64)
    b = _bisect(cdf, t, z, z + (-(-n // TILE) - 1), lambda m: np.minimum((m + 1) * TILE, n) - 1)
    return _bisect(cdf, t, b * TILE, np.minimum((b + 1) * TILE, n) - 1, lambda m: m)


def bilinear_numpy(data, x0, y0, dx, dy, px, py):
    """hm_bilinear of csrc/nbp_heatmap.h, operation for operation (points inside the box)"""
    nx, ny = data.shape
    fx, fy = (px - x0) / dx, (py - y0) / dy
    i0, j0 = np.minimum(fx.astype(np.int64), nx - 2), np.minimum(fy.astype(np.int64), ny - 2)
    tx, ty = fx - i0.astype(np.float64), fy - j0.astype(np.float64)
    a = (1.0 - ty) * data[i0, j0] + ty * data[i0, j0 + 1]
    b = (1.0 - ty) * data[i0 + 1, j0] + ty * data[i0 + 1, j0 + 1]
    return (1.0 - tx) * a + tx * b


def check_grid(data, x, y, bw_factor):
    """step 1: what nbp_heatmap_create refuses, raised here as ValueError -> (data, x, y, dx, dy, h)"""
    data = np.ascontiguousarray(data, dtype=np.float64)
    x, y = np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if data.ndim != 2 or data.shape != (x.size, y.size):
        raise ValueError("heatmap: data must be len(x) by len(y)")
    if x.size < 2 or y.size < 2:
        raise ValueError("heatmap: nx, ny >= 2")
    if data.size > MAX_CELLS:
        raise ValueError("heatmap: more than 2^26 cells")
    sp = []
    for name, v in (("x", x), ("y", y)):
        s = (v[-1] - v[0]) / np.float64(v.size - 1)
        df = np.diff(v)
        if not (np.isfinite(v[0]) and np.isfinite(s) and s > 0 and np.all(df > 0) and np.all(np.abs(df - s) <= 1e-9 * abs(s))):
            raise ValueError(f"heatmap: {name} is not strictly increasing with uniform spacing")
        sp.append(s)
    if not np.all(np.isfinite(data)):
        raise ValueError("heatmap: the field holds a value that is not finite")
    if not np.any(data > 0):
        raise ValueError("heatmap: no positive cell")
    if not (np.isfinite(bw_factor) and bw_factor > 0):
        raise ValueError("heatmap: bw_factor must be positive and finite")
    return data, x, y, sp[0], sp[1], np.float64(bw_factor) * 0.5 * (sp[0] + sp[1])


def heatmap_density_numpy(data, x, y, bw_factor=0.7, M=10000, n=None, seed=0, seed2=None, jitter=0):
    """steps 1-7 on the host -> a dict of every stage: h, bw, cdf, total, t (= ua * total per pre-sample), cell, pre (M x 2), d, W,
    wcdf, wtotal, tw (= ua * wtotal per draw), pick, points (n x 2).  n defaults to M, seed2 to seed."""
    data, x, y, dx, dy, h = check_grid(data, x, y, bw_factor)
    M = int(M)
    n = M if n is None else int(n)
    if M < 1 or n < 1:
        raise ValueError("heatmap: M, n >= 1")
    seed2 = seed if seed2 is None else seed2
    nx, ny = data.shape
    flat = data.reshape(-1)
    cdf = scan_numpy(np.where(flat > 0, flat, 0.0))
    total = cdf[-1]
    m = np.arange(M)
    ua, _ = uniform_pairs(seed, m, PURP_HMCELL, 0)
    t = ua * total
    cell = search_numpy(cdf, t)
    for q in np.flatnonzero(~(flat[cell] > 0)):  # (a cell of weight 0: only where the sums' last bits are not monotone)
        c = cell[q]
        while c < flat.size - 1 and not flat[c] > 0:
            c += 1
        cell[q] = c if flat[c] > 0 else np.flatnonzero(flat > 0)[-1]
    i, j = cell // ny, cell % ny
    n0, n1 = normal_pairs(seed, m, PURP_HMNOISE, 0)
    px, py = x[i] + h * n0, y[j] + h * n1
    inside = (px >= x[0]) & (px <= x[-1]) & (py >= y[0]) & (py <= y[-1])
    d = np.zeros(M)
    d[inside] = bilinear_numpy(data, x[0], y[0], dx, dy, px[inside], py[inside])
    W = np.exp(np.maximum(-(d - d.min()), -700.0))
    wcdf = scan_numpy(W)
    wtotal = wcdf[-1]
    k = np.arange(n)
    ua2, _ = uniform_pairs(seed2, k, PURP_HMPICK, 0)
    tw = ua2 * wtotal
    pick = search_numpy(wcdf, tw)
    pre = np.stack([px, py], axis=1)
    points = pre[pick].copy()
    if jitter:
        j0, j1 = normal_pairs(seed2, k, PURP_HMNOISE, 1)
        points[:, 0] = points[:, 0] + h * j0
        points[:, 1] = points[:, 1] + h * j1
    return dict(h=h, bw=np.array([h, h]), dx=dx, dy=dy, cdf=cdf, total=total, t=t, cell=cell.astype(np.int32), pre=pre, inside=inside,
                d=d, W=W, wcdf=wcdf, wtotal=wtotal, tw=tw, pick=pick.astype(np.int32), points=points)


# ---- the classes ------------------------------------------------------------------------------------------------------------------
def _device(backend, n, method):
    """the HIP backend a heatmap density is built or evaluated on (None: HipBackend), holding n points (at most MAXN)"""
    return _backend(backend, min(int(n), abi.MAXN), 1, method, required="heatmap densities are computed by libnbp")


class HeatmapGridDensity:
    """HeatmapGridDensity(field_on_grid, domain, hint_callback, bw_factor; N) (ext/HeatmapSampler.jl:162-210).  domain = (x, y);
    N pre-samples; the density is `points` (n x 2, n defaults to N) with bandwidth `bw` = (h, h), built by libnbp
    (nbp_heatmap_create / _build / _draw) on `backend` -- a HIP backend class, factory or instance; None: HipBackend."""

    def __init__(self, data, domain, hint_callback=None, bw_factor=0.7, N=10000, n=None, seed=0, backend=None):
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.domain = (np.ascontiguousarray(domain[0], dtype=np.float64), np.ascontiguousarray(domain[1], dtype=np.float64))
        self.hint_callback, self.bw_factor, self.N, self.seed = hint_callback, float(bw_factor), int(N), int(seed)
        self._backend = backend
        n = self.N if n is None else int(n)
        _, self.points, self.bw = self._draw(n, self.seed, 0)

    def _draw(self, n, seed, jitter):
        with _device(self._backend, n, "heatmap_create") as be:
            hm = be.heatmap_create(self.data, self.domain[0], self.domain[1], self.bw_factor)
            try:
                be.heatmap_build(hm, self.N, self.seed, outputs=False)
                return be.heatmap_draw(hm, n, seed, jitter=jitter)
            finally:
                be.heatmap_destroy(hm)

    def __call__(self, pts, backend=None):
        """hgd(pts): the density of (points, bw) at pts (q x 2), through kde_evaluate -- a context holds at most N points of a
        belief, so the points go in runs of N and the runs' densities are averaged by their share of the points"""
        with _device(self._backend if backend is None else backend, len(self.points), "kde_evaluate") as be:
            Q, n = np.asarray(pts, dtype=np.float64).reshape(-1, 2), len(self.points)
            return sum(be.kde_evaluate(abi.EUCLID2, self.points[a:a + be.N], self.bw, Q) * (min(be.N, n - a) / n) for a in range(0, n, be.N))

    def sample(self, n, seed=0):
        """AMP.sample(hgd, n): n draws of pre-sample + h * randn (rebuilds the pre-samples of the construction: same seed, same M)"""
        return self._draw(int(n), int(seed), 1)[1]


class LevelSetGridNormal:
    """LevelSetGridNormal(field_on_grid, domain, level, sigma; sigma_scale, hint_callback, bw_factor, N), the reference's legacy
    constructor (ext/HeatmapSampler.jl:229-242): it builds the HeatmapGridDensity of the field (`.heatmap`) and carries `level`,
    `sigma` and `sigma_scale` along.  As in the reference, the three do not shape the density."""

    def __init__(self, data, domain, level, sigma, sigma_scale=3, hint_callback=None, bw_factor=0.7, N=10000, n=None, seed=0,
                 backend=None):
        self.level, self.sigma, self.sigma_scale = float(level), float(sigma), float(sigma_scale)
        self.heatmap = HeatmapGridDensity(data, domain, hint_callback, bw_factor, N=N, n=n, seed=seed, backend=backend)

    def __call__(self, pts, backend=None):
        return self.heatmap(pts, backend=backend)


def sample(Z, n, seed=0):
    """sample(hgd, n, seed): the jittered draw, of either class"""
    return getattr(Z, "heatmap", Z).sample(n, seed)


__all__ = ["HeatmapGridDensity", "LevelSetGridNormal", "sample", "heatmap_density_numpy", "scan_numpy", "search_numpy", "bilinear_numpy",
           "uniform_pairs", "normal_pairs", "check_grid"]
