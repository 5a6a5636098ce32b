"""Scene densities: every belief of a graph on ONE regular grid -- the picture of a whole solution.

  plotKDE / plotSLAM2D over all variables     what a user of the reference draws first after a solve: every pose and every
                                              landmark cloud on one map (one host KDE per variable there, overlaid)
  sceneGrid(fg)                               the same picture from one call: S = sum_v w_v p_v on a common grid, and under every
                                              pixel the variable that owns it

The definition ("Scene densities"; defined here, unpinned: DESIGN.md 8).  A list of V beliefs, belief v with c_v points
on its manifold, bandwidth bw_v, one or two coordinates dims_v and a weight w_v >= 0; ADMISSIBLE: every belief names as many
coordinates as belief 0 and, axis by axis, the same kind (Euclidean or circular) -- an SE(2) pose on (x, y) beside a Euclid(2)
landmark is.  USABLE: the bandwidth entries on dims_v are positive and finite; an unusable belief adds nothing and is reported.

  box       per axis a, d = dims_v[a], h = bw_v[d], mn / mx the minimum / maximum of the belief's points on d:
            cull_lo = mn - reach h, cull_hi = mx + reach h, ext_lo = mn - margin h, ext_hi = mx + margin h
  grid      point k of axis a = lo_a + float(k) step_a, row-major, axis 0 slowest.  Automatic extent: a Euclidean axis has lo = min
            ext_lo and hi = max ext_hi over the usable beliefs, step = (hi - lo) / (n - 1) (no usable belief: lo = step = 0); a
            circular axis lo = -pi, step = 2 pi / n.
  in reach  belief v is in reach of a grid point when cull_lo <= g <= cull_hi on every Euclidean axis; circular axes never cull;
            reach = inf puts every belief in reach of every point
  value     S[k0][k1] = sum_v w_v (P_v / norm_v) over the usable beliefs in reach of the point, in list order, P_v and norm_v the sum
            and the normalisation of `marginal_grid_numpy`; a point no belief reaches is exactly 0.0
  owner     the list index of the largest term w_v (P_v / norm_v) > 0 among the beliefs in reach, ties to the lower index; -1: none
  bound     a belief out of reach of a point has every particle further than reach h from it on some axis: each term left out is
            below w_v exp(-reach^2 / 2) / prod_a (sqrt(2 pi) h_a)  (`truncation_bound`)

COORDINATES.  `HipBackend.run_scene_grid` and the numpy restatements count coordinates from 0; `sceneGrid` and
`SolveSession.sceneGrid` count from 1, like `marginalGrid`.

On a HIP backend the whole list is one launch sequence (csrc/nbp_scene.h): a record per belief, the extent, then one wave per 32 x 32
tile that walks the records, works only on the beliefs whose box meets the tile, and adds in list order; one grid comes back.
`scene_grid_numpy` and `scene_extent_numpy` restate the definition on the host with the exact sums of `marginal_grid_numpy`; they
serve tests, readers and callers without a HIP backend, and are never a fallback on one."""
import math
import re

import numpy as np

from . import abi
from .beliefquery import _bw, _manifold, _staged
from .marginal import _axis_table, _dims0, _norm, grid_axes
from .ppe import _circular, _natural, ppe_coords

SCENE_MAX, REACH, MARGIN = abi.SCENE_MAX, abi.SCENE_REACH, abi.SCENE_MARGIN


# ------------------------------------------------------------------------------------------------
# the definition on the host
# ------------------------------------------------------------------------------------------------
def _prepare(beliefs):
    """beliefs = [(manifold, X (c x D tangent coordinates), bw, dims 0-based)] -> [(X, bw padded to D, dims, kinds, usable)];
    ValueError where the list is not admissible"""
    out = []
    for v, (m, X, bw, dims) in enumerate(beliefs):
        D = abi.MANIFOLD_DIM[m]
        X = np.asarray(X, dtype=np.float64).reshape(-1, D)
        dims = _dims0(m, dims)
        circ = _circular(m)
        kinds = [circ[d] for d in dims]
        h = _bw(m, bw)
        usable = all(np.isfinite(h[d]) and h[d] > 0 for d in dims)
        if out and kinds != out[0][3]:
            raise ValueError(f"scene: belief {v} is not admissible against belief 0: the coordinates differ in number or kind")
        out.append((X, h, dims, kinds, usable))
    return out


def _sizes(n, axes):
    n = [int(v) for v in np.atleast_1d(n)]
    n = n * axes if len(n) == 1 else n
    if len(n) != axes or min(n) < 1 or max(n) > SCENE_MAX or int(np.prod(n)) > abi.SCENE_MAX_POINTS:
        raise ValueError(f"scene: one size within 1..{SCENE_MAX} per axis, at most 2^22 points")
    return n


def _box(X, h, dims, a, by):
    """(min - by h, max + by h) of axis a, as written"""
    d = dims[a]
    with np.errstate(invalid="ignore"):
        return X[:, d].min() - by * h[d], X[:, d].max() + by * h[d]


def _extent(prep, n, margin):
    margin = np.float64(margin)
    ext = np.zeros(4)
    if not prep:
        return ext
    use = [p for p in prep if p[4]]
    for a, circ in enumerate(prep[0][3]):
        if circ:
            ext[2 * a], ext[2 * a + 1] = -np.pi, (2 * np.pi) / np.float64(n[a])
            continue
        if n[a] < 2:
            raise ValueError("the automatic extent of a Euclidean axis needs n >= 2")
        if use:
            boxes = [_box(X, h, dims, a, margin) for X, h, dims, _, _ in use]
            lo, hi = min(b[0] for b in boxes), max(b[1] for b in boxes)
            ext[2 * a], ext[2 * a + 1] = lo, (hi - lo) / np.float64(n[a] - 1)
    return ext


def scene_extent_numpy(beliefs, n, margin=MARGIN):
    """the automatic extent of a scene, in the written order of the definition: beliefs = [(manifold, X (c x D tangent coordinates),
    bw, dims 0-BASED)] -> [lo0, step0, lo1, step1] (1-D: lo1 = step1 = 0)"""
    prep = _prepare(beliefs)
    return _extent(prep, _sizes(n, len(prep[0][2]) if prep else len(np.atleast_1d(n))), margin)


def truncation_bound(bw, dims, reach, weight=1.0):
    """what one belief out of reach of a grid point would have added there, at most"""
    return float(weight) * math.exp(-0.5 * float(reach) ** 2) / float(np.prod([math.sqrt(2 * math.pi) * bw[d] for d in dims]))


def scene_grid_numpy(beliefs, n, lo=None, step=None, margin=MARGIN, reach=REACH, weights=None, owner=False, terms=False, exact=True):
    """the scene of the definition: beliefs = [(manifold, X (c x D tangent coordinates), bw, dims 0-BASED)], n the points per axis;
    lo and step per axis, or neither for the automatic extent with `margin`; weights: one per belief (None: all 1) ->
    (grid (n0,) or (n0, n1), extent [lo0, step0, lo1, step1], owner grid (int32; None unless `owner`), skipped[V]); with `terms` a
    fifth entry: the V terms w_v (P_v / norm_v) stacked, zero where a belief is out of reach.  The sums over j are exact
    (math.fsum, as in `marginal_grid_numpy`); exact=False: numpy's matrix product, for large scenes."""
    prep = _prepare(beliefs)
    V = len(prep)
    axes = len(prep[0][2]) if V else len(np.atleast_1d(n))
    n = _sizes(n, axes)
    if (lo is None) != (step is None):
        raise ValueError("scene: lo and step come together")
    if lo is None:
        ext = _extent(prep, n, margin)
    else:
        ext = np.zeros(4)
        lo, step = np.atleast_1d(lo).astype(np.float64), np.atleast_1d(step).astype(np.float64)
        if not (np.all(np.isfinite(lo[:axes])) and np.all(np.isfinite(step[:axes]) & (step[:axes] > 0))):
            raise ValueError("scene: lo finite, step finite and positive")
        for a in range(axes):
            ext[2 * a], ext[2 * a + 1] = lo[a], step[a]
    w = np.ones(V) if weights is None else np.asarray(weights, dtype=np.float64).reshape(V)
    if not np.all(np.isfinite(w) & (w >= 0)):
        raise ValueError("scene: weights are finite and not negative")
    if not (reach > 0):
        raise ValueError("scene: reach is positive (inf: no culling)")
    shape, G, reach = tuple(n), grid_axes(ext, n), np.float64(reach)
    S = np.zeros(shape)
    best, own = np.zeros(shape), np.full(shape, -1, dtype=np.int32)
    skipped = np.zeros(V, dtype=np.int32)
    stack = np.zeros((V,) + shape) if terms else None
    for v, (X, h, dims, kinds, usable) in enumerate(prep):
        if not usable:
            skipped[v] = 1
            continue
        inr = []
        for a, circ in enumerate(kinds):
            cl, ch = _box(X, h, dims, a, reach)
            inr.append(np.ones(n[a], dtype=bool) if circ else (cl <= G[a]) & (G[a] <= ch))
        if not all(i.any() for i in inr):
            continue
        norm = _norm(X.shape[0], h, dims)
        E0 = _axis_table(G[0][inr[0]], X[:, dims[0]], kinds[0], h[dims[0]])
        if axes == 1:
            P = np.array([math.fsum(r) for r in E0.tolist()]) if exact else E0.sum(axis=1)
            where = inr[0]
        else:
            E1 = _axis_table(G[1][inr[1]], X[:, dims[1]], kinds[1], h[dims[1]])
            if exact:
                P = np.zeros((E0.shape[0], E1.shape[0]))
                for k0 in range(E0.shape[0]):
                    P[k0] = [math.fsum(r) for r in (E0[k0][None, :] * E1).tolist()]
            else:
                P = E0 @ E1.T
            where = np.ix_(inr[0], inr[1])
        term = np.zeros(shape)
        term[where] = w[v] * (P / norm)
        S = S + term
        if owner:
            m = term > best
            best[m], own[m] = term[m], v
        if terms:
            stack[v] = term
    res = (S, ext, own if owner else None, skipped)
    return res + (stack,) if terms else res


# ------------------------------------------------------------------------------------------------
# the graph-level call
# ------------------------------------------------------------------------------------------------
class Scene:
    """sceneGrid's result: `grid` (n0,) or (n0, n1), axis 0 = the first coordinate of `dims`; `axes` the coordinate vectors; `extent`
    [lo0, step0, lo1, step1] as used; `labels` the variables in list order; `owner` the grid of list indices (None unless asked
    for; -1: nobody); `skipped` the labels whose bandwidth was unusable; `tile_beliefs` the (tile, belief) pairs the device worked
    on (None on the host route).  `.at(x[, y])`: the label that owns the pixel nearest to a location."""

    def __init__(self, grid, axes, extent, labels, owner, skipped, tile_beliefs):
        self.grid, self.axes, self.extent, self.labels = grid, axes, np.asarray(extent), list(labels)
        self.owner, self.skipped, self.tile_beliefs = owner, list(skipped), tile_beliefs

    def index(self, *loc):
        """the index of the grid point nearest to a location, or None outside the grid"""
        if len(loc) != self.grid.ndim:
            raise ValueError(f"a location of this scene has {self.grid.ndim} coordinates")
        k = []
        for a, x in enumerate(loc):
            lo, st = self.extent[2 * a], self.extent[2 * a + 1]
            i = int(round((float(x) - lo) / st)) if st > 0 else 0
            if not 0 <= i < self.grid.shape[a]:
                return None
            k.append(i)
        return tuple(k)

    def at(self, *loc):
        """the label of the variable under a location (the owner of the nearest pixel); None where nobody is, or outside the grid"""
        if self.owner is None:
            raise ValueError("this scene was made without owners: sceneGrid(..., owner=True)")
        k = self.index(*loc)
        if k is None or self.owner[k] < 0:
            return None
        return self.labels[int(self.owner[k])]


def scene_labels(fg, labels, dims):
    """(labels, {label: 1-based dims}) of a scene: labels a list, a regular expression (as in findVariablesNear) or None for every
    initialised variable that has the coordinates; dims one tuple for all or a dict {label: dims}"""
    per = dims if isinstance(dims, dict) else None
    one = None if per is not None else tuple(int(d) for d in np.atleast_1d(dims))

    def of(v):
        if per is None:
            return one
        if v not in per:
            raise ValueError(f"scene: no coordinates given for {v}")
        return tuple(int(d) for d in np.atleast_1d(per[v]))

    if labels is None or isinstance(labels, (str, re.Pattern)):
        rx = None if labels is None else (re.compile(labels) if isinstance(labels, str) else labels)
        labels = [v for v in sorted(fg.ls(), key=_natural)
                  if (rx is None or rx.search(v)) and fg.getVariable(v).initialized and (per is None or v in per)
                  and fg.getVariable(v).varType.dim >= max(of(v))]
    else:
        labels = list(labels)
    return labels, {v: of(v) for v in labels}


def scene_columns(fg, labels, dims_of, weights, place):
    """(slots, manifolds, 0-based dims V x k, weights or None) of run_scene_grid; ValueError where the list is not admissible"""
    mans = [_manifold(fg.getVariable(v).varType) for v in labels]
    dd = [_dims0(m, [d - 1 for d in dims_of[v]]) for v, m in zip(labels, mans)]
    kinds = [[_circular(m)[d] for d in ds] for m, ds in zip(mans, dd)]
    for v, k in zip(labels, kinds):
        if k != kinds[0]:
            raise ValueError(f"sceneGrid: {v} cannot be drawn with {labels[0]}: the coordinates differ in number or kind")
    if isinstance(weights, dict):
        w = [float(weights.get(v, 1.0)) for v in labels]
    else:
        w = None if weights is None else [float(x) for x in weights]
    return [place[v] for v in labels], mans, dd, w


def scene_from_result(labels, n, res, tile_beliefs=None):
    grid, ext, own, skipped = res[:4]
    return Scene(grid, grid_axes(ext, list(grid.shape)), ext, labels, own, [v for v, s in zip(labels, skipped) if s], tile_beliefs)


def sceneGrid(fg, labels=None, dims=(1, 2), n=512, extent=None, margin=MARGIN, reach=REACH, weights=None, owner=False, backend=None):
    """The current beliefs of the variables `labels` on ONE grid -> Scene(grid, axes, extent, labels, owner, skipped, tile_beliefs).
    labels: a list, a regular expression (as in findVariablesNear), or None for every initialised variable that has the coordinates;
    dims: one or two coordinates, 1-BASED like `marginalGrid`, or a dict {label: dims}; n: points per axis (a scalar: the same on
    both); extent = ((lo0, step0)[, (lo1, step1)]) or None for the automatic one with `margin`; reach: how many bandwidths beyond its
    cloud a belief is drawn (inf: everywhere); weights: a dict {label: w} (default 1) or one per label; owner: also the grid of
    owners, for `.at(x, y)`.  `backend`: a HIP backend (class, factory or instance: the beliefs go to slots once and ONE
    run_scene_grid draws them all); None: numpy (scene_grid_numpy)."""
    labels, dims_of = scene_labels(fg, labels, dims)
    if not labels:
        raise ValueError("sceneGrid: no variable to draw")
    place = {v: i for i, v in enumerate(labels)}
    slots, mans, dd, w = scene_columns(fg, labels, dims_of, weights, place)
    nn = _sizes(n, len(dd[0]))
    e = None if extent is None else np.asarray(extent, dtype=np.float64).reshape(-1)
    if e is not None and e.size != 2 * len(nn):
        raise ValueError("an extent is (lo, step) per axis")
    with _staged(fg, labels, backend, "run_scene_grid", _bw) as (be, _):
        if be is not None:
            *res, tb = be.run_scene_grid(slots, mans, dd, nn, e, margin, reach, w, owner)
            return scene_from_result(labels, nn, res, tb)
    var = fg.getVariable
    bel = [(m, ppe_coords(m, var(v).val), var(v).bw, ds) for v, m, ds in zip(labels, mans, dd)]
    lo, step = (None, None) if e is None else (e[0::2].copy(), e[1::2].copy())
    return scene_from_result(labels, nn, scene_grid_numpy(bel, nn, lo, step, margin, reach, w, owner))
