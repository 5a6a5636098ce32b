"""Marginal densities of a belief: on a regular grid over one or two of its coordinates, and at query points.

  plotKDE / plotPose marginals          what every user of the reference looks at: the x-y picture of a pose with the heading
                                        integrated out, the 1-D picture of one coordinate
  getBelief of a partial belief         propagateBelief over a lone PartialPriorPassThrough leaves bandwidth (h0, h1, 0)
                                        (test/testSpecialEuclidean2Mani.jl:331-370): a density on the partial coordinates

The definitions ("Marginal densities"), for a belief of c points x_j on a manifold of dimension D with bandwidth h, in
tangent coordinates at the identity (SE(2): x, y, theta), and a coordinate set K of one or more coordinates:

  marginal  p_K(q) = 1 / (c prod_{d in K} sqrt(2 pi) h_d) * sum_{j < c} exp(-1/2 sum_{d in K} (delta_d(q, x_j) / h_d)^2), delta
            wrapped to [-pi, pi) on circular coordinates: `density_numpy`'s density with the coordinates outside K dropped --
            integrating a coordinate out of a product-kernel KDE is dropping it.  Only the bandwidth entries in K must be positive
            and finite (else every value is NaN); the others are not looked at.
  grid      1-D or 2-D; point k of axis a is lo_a + float(k) * step_a (one multiplication, one addition), n_a points per axis,
            1 <= n_a <= GRID_MAX; the output is row-major, the first listed coordinate slowest.
            E_a[k][j] = exp(-1/2 (((g_a[k] - x_j[d_a]) wrapped where circular) * (1 / h_a))^2);
            value = (sum_j E_0[k0][j] * E_1[k1][j]) / norm (1-D: (sum_j E_0[k0][j]) / norm), norm = c * prod sqrt(2 pi) h_d over K
            in ascending coordinate order: dims = (b, a) gives the transpose of dims = (a, b) bit for bit.
  extent    automatic: a Euclidean axis lo = min_j x - margin h, hi = max_j x + margin h, step = (hi - lo) / (n - 1) (n >= 2); a
            circular axis lo = -pi, step = 2 pi / n (margin plays no part).

COORDINATES.  The C ABI, `HipBackend.run_marginal_grid` / `kde_marginal_grid` / `run_evaluate_marginal` and the numpy restatements
here count coordinates from 0.  `Belief.marginal`, `marginalGrid` and `SolveSession.marginalGrid` -- the names a user of the
reference calls -- count from 1, like the reference's `partial`.

Defined here and unpinned against KernelDensityEstimate.jl, like the density they extend.  On a HIP backend a grid is
one workgroup per 32 x 32 tile with the exponentials shared along each axis (csrc/nbp_marginal.h); `marginal_grid_numpy` and
`marginal_density_numpy` restate the definitions on the host with exact sums."""
import math

import numpy as np

from . import abi
from .beliefquery import Belief, _backend, _manifold, _wrap
from .ppe import _circular, ppe_coords

GRID_MAX = abi.GRID_MAX
_SQRT_2PI = math.sqrt(2.0 * math.pi)


def _dims0(manifold, dims):
    """0-based coordinates as a list of one or two distinct coordinates of the manifold"""
    dims = [int(d) for d in np.atleast_1d(dims)]
    D = abi.MANIFOLD_DIM[manifold]
    if len(dims) not in (1, 2) or len(set(dims)) != len(dims) or min(dims) < 0 or max(dims) >= D:
        raise ValueError(f"marginal: one or two distinct coordinates within 0..{D - 1}, got {dims}")
    return dims


def _norm(c, bw, dims):
    norm = float(c)
    for d in sorted(dims):
        norm *= _SQRT_2PI * bw[d]
    return norm


def grid_extent_numpy(manifold, X, bw, dims, n, margin=4.0):
    """the automatic extent, in the written order of the definition -> [lo0, step0, lo1, step1] (1-D: lo1 = step1 = 0)"""
    D = abi.MANIFOLD_DIM[manifold]
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    dims, n = _dims0(manifold, dims), [int(v) for v in np.atleast_1d(n)]
    circ, margin = _circular(manifold), np.float64(margin)
    ext = np.zeros(4)
    for a, d in enumerate(dims):
        if circ[d]:
            ext[2 * a], ext[2 * a + 1] = -np.pi, (2 * np.pi) / np.float64(n[a])
        else:
            if n[a] < 2:
                raise ValueError("the automatic extent of a Euclidean axis needs n >= 2")
            lo, hi = X[:, d].min() - margin * bw[d], X[:, d].max() + margin * bw[d]
            with np.errstate(invalid="ignore"):
                ext[2 * a], ext[2 * a + 1] = lo, (hi - lo) / np.float64(n[a] - 1)
    return ext


def grid_axes(extent, n):
    """the coordinate vectors of a grid: point k of axis a = lo_a + float(k) * step_a"""
    n = [int(v) for v in np.atleast_1d(n)]
    return [extent[2 * a] + np.arange(n[a], dtype=np.float64) * extent[2 * a + 1] for a in range(len(n))]


def _axis_table(g, x, circ, h):
    """E[k][j] of one axis"""
    d = g[:, None] - x[None, :]
    if circ:
        d = _wrap(d)
    d = d * (1.0 / h)
    return np.exp(-0.5 * (d * d))


def marginal_grid_numpy(manifold, X, bw, dims, n, lo=None, step=None, margin=4.0):
    """the grid of the definition: X (c x D) the belief's tangent coordinates, bw its bandwidth, dims the one or two 0-BASED
    coordinates of the grid, n the points per axis; lo and step per axis (scalars or sequences), or neither for the automatic
    extent with `margin` -> (grid of shape (n0,) or (n0, n1), extent [lo0, step0, lo1, step1]).  The sums over j are exact
    (math.fsum of the separable products)."""
    D = abi.MANIFOLD_DIM[manifold]
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    dims, n = _dims0(manifold, dims), [int(v) for v in np.atleast_1d(n)]
    if len(n) != len(dims) or min(n) < 1 or max(n) > GRID_MAX:
        raise ValueError(f"marginal grid: one size within 1..{GRID_MAX} per coordinate")
    if (lo is None) != (step is None):
        raise ValueError("marginal grid: lo and step come together")
    if lo is None:
        ext = grid_extent_numpy(manifold, X, bw, dims, n, margin)
    else:
        ext = np.zeros(4)
        lo, step = np.atleast_1d(lo).astype(np.float64), np.atleast_1d(step).astype(np.float64)
        for a in range(len(dims)):
            ext[2 * a], ext[2 * a + 1] = lo[a], step[a]
    shape = tuple(n)
    if len(bw) < D or not all(np.isfinite(bw[d]) and bw[d] > 0 for d in dims):
        return np.full(shape, np.nan), ext
    circ, G = _circular(manifold), grid_axes(ext, n)
    norm = _norm(X.shape[0], bw, dims)
    E0 = _axis_table(G[0], X[:, dims[0]], circ[dims[0]], bw[dims[0]])
    if len(dims) == 1:
        return np.array([math.fsum(r) for r in E0.tolist()]) / norm, ext
    E1 = _axis_table(G[1], X[:, dims[1]], circ[dims[1]], bw[dims[1]])
    out = np.zeros(shape)
    for k0 in range(n[0]):
        out[k0] = [math.fsum(r) for r in (E0[k0][None, :] * E1).tolist()]
    return out / norm, ext


def marginal_density_numpy(manifold, X, bw, dims, Q):
    """p_K at query points: X (c x D), bw, dims the 0-BASED coordinates of K (any non-empty subset), Q (q x D; the columns outside
    K are not read) -> q values.  The sum over j is exact (math.fsum)."""
    D = abi.MANIFOLD_DIM[manifold]
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, D)
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    dims = sorted({int(d) for d in np.atleast_1d(dims)})
    if not dims or dims[0] < 0 or dims[-1] >= D:
        raise ValueError(f"marginal: a non-empty set of coordinates within 0..{D - 1}")
    if len(bw) < D or not all(np.isfinite(bw[d]) and bw[d] > 0 for d in dims):
        return np.full(Q.shape[0], np.nan)
    circ = _circular(manifold)
    norm = _norm(X.shape[0], bw, dims)
    out = np.zeros(Q.shape[0])
    for i in range(Q.shape[0]):
        e = np.zeros(X.shape[0])
        for d in dims:
            dl = Q[i, d] - X[:, d]
            if circ[d]:
                dl = _wrap(dl)
            e += (dl / bw[d]) ** 2
        out[i] = math.fsum(np.exp(-0.5 * e).tolist()) / norm
    return out


def _mask(dims0):
    return sum(1 << d for d in dims0)


def _default_dims1(manifold, bw):
    """the 1-based coordinates a grid takes when none are named: the first two (or the one) the belief has a bandwidth on -- for
    a partial belief its partial coordinates"""
    D = abi.MANIFOLD_DIM[manifold]
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    have = [d + 1 for d in range(min(D, len(bw))) if np.isfinite(bw[d]) and bw[d] > 0]
    if not have:
        raise ValueError("marginal: the belief has no coordinate with a positive finite bandwidth")
    return tuple(have[:2])


def _extent_args(extent, k):
    """extent = ((lo0, step0)[, (lo1, step1)]) or flat -> (lo[k], step[k])"""
    e = np.asarray(extent, dtype=np.float64).reshape(-1)
    if e.size != 2 * k:
        raise ValueError("an extent is (lo, step) per axis")
    return e[0::2].copy(), e[1::2].copy()


class Marginal:
    """belief.marginal(dims): p_K of a belief, K = the 1-BASED coordinates `dims`.  Calling it evaluates p_K at host points;
    `.grid` evaluates it on a regular grid."""

    def __init__(self, belief, dims):
        self.belief = belief
        self.dims = tuple(int(d) for d in np.atleast_1d(dims))
        D = abi.MANIFOLD_DIM[belief.manifold]
        if not self.dims or len(set(self.dims)) != len(self.dims) or min(self.dims) < 1 or max(self.dims) > D:
            raise ValueError(f"marginal: distinct 1-based coordinates within 1..{D}, got {self.dims}")
        self._dims0 = [d - 1 for d in self.dims]

    def __call__(self, pts, backend=None):
        """densities at host points (q x P, as Belief.__call__ takes them; what they hold outside K plays no part).  `backend`: a
        HIP backend (class, factory or instance: the belief goes to slot 0, nbp_run_evaluate_marginal); else numpy."""
        b = self.belief
        Q = ppe_coords(b.manifold, np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[b.manifold]))
        with _backend(backend, len(b.pts), 1, "run_evaluate_marginal") as be:
            if be is not None:
                be.belief_write(0, b.manifold, b.pts, b.bw)
                return be.run_evaluate_marginal([0], [b.manifold], [_mask(self._dims0)], [Q])[0]
            return marginal_density_numpy(b.manifold, ppe_coords(b.manifold, b.pts), b.bw, self._dims0, Q)

    def grid(self, n, extent=None, margin=4.0, backend=None):
        """p_K on a regular grid of n points per axis (a scalar n: the same on every axis) -> (grid, axes): grid of shape (n0,) or
        (n0, n1), the first coordinate of `dims` slowest; axes = the coordinate vectors.  extent = ((lo0, step0)[, (lo1, step1)]),
        or None for the automatic extent with `margin`.  `backend` as in __call__ (nbp_kde_marginal_grid, through slot 0)."""
        b, k = self.belief, len(self.dims)
        if k > 2:
            raise ValueError("a grid has one or two coordinates")
        n = [int(v) for v in np.atleast_1d(n)]
        n = n * k if len(n) == 1 else n
        with _backend(backend, len(b.pts), 1, "kde_marginal_grid") as be:
            if be is not None:
                g, ext = be.kde_marginal_grid(b.manifold, b.pts, b.bw, self._dims0, n, extent, margin)
            else:
                lo, step = (None, None) if extent is None else _extent_args(extent, k)
                g, ext = marginal_grid_numpy(b.manifold, ppe_coords(b.manifold, b.pts), b.bw, self._dims0, n, lo, step, margin)
            return g, grid_axes(ext, n)


def marginalGrid(fg, label, dims=None, n=64, extent=None, margin=4.0, backend=None):
    """The marginal density of a variable's current belief on a regular grid -> (grid, axes).  `dims`: one or two coordinates,
    1-BASED like the reference's `partial` (the C ABI and the `HipBackend` methods count from 0); None: the first two coordinates
    the belief has a bandwidth on -- for a partial belief its partial coordinates.  n, extent, margin and backend as in
    `Marginal.grid`.  The marginal maximum is `np.unravel_index(np.argmax(grid), grid.shape)` on the host."""
    v = fg.getVariable(label)
    man = _manifold(v.varType)
    dims = _default_dims1(man, v.bw) if dims is None else dims
    return Belief(man, v.val, v.bw).marginal(dims).grid(n, extent, margin, backend)
