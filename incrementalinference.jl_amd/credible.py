"""Credible regions of a belief: how much of it lies where.

  credibleRegion(fg, "x5")           the levels of the highest-density regions (HDR) at masses 0.5 / 0.9 / 0.95 and the quantiles
                                     of every coordinate
  credibility(fg, {"x5": truth})     the mass of the smallest HDR that still contains a reference point: is the ground truth (or a
                                     candidate landmark position) inside the 90 % region of the belief?
  coverage(masses)                   the calibration table: the share of reference points inside the 50 / 90 / 95 % regions

The reference has no such query: its beliefs are multimodal by design, where a covariance ellipse or a NEES test means nothing,
and its own tests note that the product is over-confident (test/testBasicGraphs.jl:89,110).  DEFINED here and unpinned (DESIGN.md
3, "Credible regions", and 8).  For a belief of c points x_i on a manifold of dimension D with bandwidth h, in tangent coordinates at
the identity (SE(2): x, y, theta), and a non-empty set K of coordinates (the 1-BASED `dims`, like `marginalGrid`; default all):

  l_i        M_i + log(sum_{j != i} exp(e_ij - M_i)) - log((c - 1) prod_{d in K} sqrt(2 pi) h_d), e_ij = -1/2 sum_{d in K}
             (delta_d(x_i, x_j) r_d)^2 with r_d = 1 / h_d and delta wrapped to [-pi, pi) on circular coordinates, M_i = max_{j != i}
             e_ij: the LEAVE-ONE-OUT log density of each own point.  Exclusion is by index: a duplicate of x_i stays in.  Finite where
             every term underflows.  (With the self term in, a tail particle's density is mostly its own kernel and the regions
             come out too small: tests/credible_cases.py holds the figures.)
  order      the particle indices by ascending (l_i, i): np.lexsort((arange(c), l))
  level(a)   for a mass a in (0, 1]: k = ceil(a c) clamped to 1 .. c; the k-th largest l_i = l[order[c - k]].  The region is
             {x : log p_K(x) >= level}; its contour on a `marginalGrid` of the same dims lies at exp(level).
             n_inside = #{i : l_i >= level} (>= k, more only through ties)
  query q    l_q = the log density of the whole KDE at q on K (all c points, normalised by c); n_above = #{i : l_i > l_q};
             mass(q) = n_above / c: 0 at the densest place, 1.0 in the far tail; q lies inside the a-region iff l_q >= level(a)
  quantiles  of every coordinate of the manifold, whatever K; the bandwidth plays no part.  v_i = x_id (a circular coordinate:
             x_id - mean_d wrapped), sorted; t = (c - 1) p, lo = floor(t), hi = min(lo + 1, c - 1), Q = v_lo + (t - lo) (v_hi - v_lo)
             (Julia's and numpy's default, type 7; np.quantile rounds its lerp differently, so it is written out); a circular
             coordinate delivers mean_d + Q wrapped.  mean: the geodesic mean of ppe.py.
  c == 1     levels, l and masses are NaN, order = [0], every quantile is the point
  a bandwidth entry in K that is not positive and finite: levels, l and query results are NaN, order is -1; the quantiles stand

Coverage is claimed AT STATED MASSES, not as uniformity of mass(truth): in one dimension the estimated density is bumpy near the
mode and the lowest decile of the masses is over-full.

The queries run on a HIP backend (`HipBackend.run_credible`: one workgroup per belief, any number of beliefs in one launch;
csrc/nbp_credible.h); there is no host route.  `credible_numpy` restates the definition in the same order of operations for tests
and readers; it is never a fallback."""
import math
from dataclasses import dataclass

import numpy as np

from . import abi
from .beliefquery import _backend, _bw, _manifold, _staged, _wrap
from .overlap import dims_mask
from .ppe import _circular, _natural, mean_geodesic_walk, ppe_coords

_SQRT_2PI = 2.5066282746310002  # NBP_SQRT_2PI of csrc/nbp_kde.h
MASS = (0.5, 0.9, 0.95)
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def level_rank(a, c):
    """k of the definition: ceil(a c) in double as written, clamped to 1 .. c"""
    return min(max(int(math.ceil(float(a) * float(c))), 1), int(c))


def quantile_type7(v_sorted, p):
    """Q of the definition on an ascending array: one rounding per written operation"""
    c = len(v_sorted)
    t = float(c - 1) * float(p)
    lo = int(math.floor(t))
    hi = min(lo + 1, c - 1)
    return float(v_sorted[lo]) + (t - float(lo)) * (float(v_sorted[hi]) - float(v_sorted[lo]))


def _exponents(manifold, X, Q, bw, mask):
    """e(q_i, x_j) on the coordinates of `mask`, formed as nbp_kde.h forms it: (delta r_d)^2 added in ascending coordinate order"""
    circ = _circular(manifold)
    e = None
    for d in range(abi.MANIFOLD_DIM[manifold]):
        if mask >> d & 1:
            dl = Q[:, d, None] - X[None, :, d]
            if circ[d]:
                dl = _wrap(dl)
            dl = dl * (1.0 / bw[d])
            e = dl * dl if e is None else e + dl * dl
    return -0.5 * e


def _log_norm(manifold, cnt, bw, mask):
    norm = float(cnt)
    for d in range(abi.MANIFOLD_DIM[manifold]):
        if mask >> d & 1:
            norm *= _SQRT_2PI * bw[d]
    return math.log(norm)


def _log_sum(e):
    """M + log(sum exp(e - M)) per row, the sum exact (math.fsum); entries of -inf are the points left out"""
    M = e.max(axis=1)
    w = np.exp(e - M[:, None])
    return M + np.log(np.array([math.fsum(r) for r in w.tolist()]))


def log_density_loo_numpy(manifold, X, bw, mask, self_term=False):
    """l_i of the definition for tangent coordinates X (c x D), c >= 2; self_term=True: the variant with the self term in and the
    normalisation c (what the definition is NOT: the calibration test shows that it fails)"""
    c = X.shape[0]
    e = _exponents(manifold, X, X, bw, mask)
    if not self_term:
        e[np.arange(c), np.arange(c)] = -np.inf
    return _log_sum(e) - _log_norm(manifold, c if self_term else c - 1, bw, mask)


def log_density_numpy(manifold, X, bw, mask, Q):
    """l_q of the definition at the rows of Q (q x D)"""
    if Q.shape[0] == 0:
        return np.zeros(0)
    return _log_sum(_exponents(manifold, X, Q, bw, mask)) - _log_norm(manifold, X.shape[0], bw, mask)


@dataclass
class CredibleNumpy:
    """what credible_numpy returns: the fields of the device's records, entry for entry"""
    logdens: np.ndarray
    order: np.ndarray
    log_levels: np.ndarray
    n_inside: np.ndarray
    log_min: float
    log_max: float
    quantiles: np.ndarray
    mean: np.ndarray
    count: int
    q_logdens: np.ndarray
    q_n_above: np.ndarray
    q_mass: np.ndarray


def credible_numpy(manifold, pts, bw, mask, mass=MASS, probs=PROBS, queries=None, mean=None):
    """The definition on the host, in the device's order of operations: pts host points (c x P), bw the bandwidth (D entries; only
    those in `mask` are looked at), mask the 0-based coordinate bit mask, queries tangent coordinates (q x D) or None -> CredibleNumpy.
    `mean`: the circular deviations are taken about this mean (a test hands in the device's) instead of the geodesic walk's."""
    X = np.ascontiguousarray(ppe_coords(manifold, pts), dtype=np.float64)
    D, c = abi.MANIFOLD_DIM[manifold], X.shape[0]
    mask = int(mask)
    if mask <= 0 or mask >> D:
        raise ValueError(f"credible: a non-empty coordinate mask inside the manifold's {D} coordinates, got {mask}")
    mass, probs = np.asarray(mass, dtype=np.float64).reshape(-1), np.asarray(probs, dtype=np.float64).reshape(-1)
    circ = _circular(manifold)
    Q = np.zeros((0, D)) if queries is None else np.asarray(queries, dtype=np.float64).reshape(-1, D)
    bw = _bw(manifold, bw)
    if mean is None:
        mean = np.array([mean_geodesic_walk(X[:, d], circ[d]) for d in range(D)])
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)[:D].copy()
    valid = all(np.isfinite(bw[d]) and bw[d] > 0 for d in range(D) if mask >> d & 1)
    levels = valid and c >= 2
    nq = Q.shape[0]
    if levels:
        l = log_density_loo_numpy(manifold, X, bw, mask)
        order = np.lexsort((np.arange(c), l)).astype(np.int32)
        ls = l[order]
        log_levels = np.array([ls[c - level_rank(a, c)] for a in mass])
        n_inside = np.array([int((l >= lev).sum()) for lev in log_levels], dtype=np.int32)
        log_min, log_max = float(ls[0]), float(ls[-1])
    else:
        l = np.full(c, np.nan)
        order = (np.arange(c) if valid else np.full(c, -1)).astype(np.int32)
        log_levels, n_inside = np.full(len(mass), np.nan), np.zeros(len(mass), dtype=np.int32)
        log_min = log_max = math.nan
    q_l = log_density_numpy(manifold, X, bw, mask, Q) if valid else np.full(nq, np.nan)
    if levels:
        q_above = np.array([int((l > v).sum()) for v in q_l], dtype=np.int32)
        q_mass = q_above.astype(np.float64) / float(c)
    else:
        q_above, q_mass = np.full(nq, -1, dtype=np.int32), np.full(nq, np.nan)
    quant = np.zeros((D, len(probs)))
    for d in range(D):
        v = _wrap(X[:, d] - mean[d]) if circ[d] else X[:, d]
        vs = v[np.lexsort((np.arange(c), v))]
        for k, p in enumerate(probs):
            q = quantile_type7(vs, p)
            quant[d, k] = float(_wrap(mean[d] + q)) if circ[d] else q
    return CredibleNumpy(l, order, log_levels, n_inside, log_min, log_max, quant, mean, c, q_l, q_above, q_mass)


def coverage(masses, at=MASS):
    """The calibration table: the fraction of `masses` (credibility masses of reference points, e.g. of the ground truth of every
    variable) that are <= a, for every a of `at` -> array.  A belief that means what it claims has coverage(a) ~ a.  NaN masses
    (beliefs without levels) are left out."""
    rows = [np.atleast_1d(np.asarray(getattr(x, "mass", x), dtype=np.float64)).reshape(-1)
            for x in (masses.values() if isinstance(masses, dict) else np.atleast_1d(masses))]
    m = np.concatenate(rows) if rows else np.zeros(0)
    m = m[~np.isnan(m)]
    return np.array([float((m <= a).mean()) if m.size else math.nan for a in np.atleast_1d(at)])


# ------------------------------------------------------------------------------------------------
# the queries on the device
# ------------------------------------------------------------------------------------------------
@dataclass
class CredibleRegion:
    """The credible regions of one belief: `log_levels[a]` / `levels[a]` (= exp) the density level of the HDR at `mass[a]`, `n_inside[a]`
    the particles at or above it; `quantiles[d, p]` the quantile of coordinate d at `probs[p]`; `mean[D]`; `count`; `logdens[c]` the
    leave-one-out log density of every particle and `order[c]` the particle indices by ascending (logdens, index)"""
    mass: np.ndarray
    log_levels: np.ndarray
    levels: np.ndarray
    n_inside: np.ndarray
    probs: np.ndarray
    quantiles: np.ndarray
    mean: np.ndarray
    count: int
    logdens: np.ndarray
    order: np.ndarray

    def inside(self, a):
        """the boolean particle mask `logdens >= level` of the region at mass `a` (one of `mass`)"""
        hit = np.flatnonzero(self.mass == float(a))
        if hit.size == 0:
            raise KeyError(f"no level at mass {a}: this CredibleRegion holds {self.mass.tolist()}")
        return self.logdens >= self.log_levels[hit[0]]


@dataclass
class Credibility:
    """The credibility of reference points under one belief: `mass` of the smallest HDR that still contains the point (0: the
    densest place, 1.0: the far tail), `logdens` the log density there, `n_above` the particles whose leave-one-out log density is
    higher.  Scalars for one point, arrays for several."""
    mass: object
    logdens: object
    n_above: object


def region_from_records(manifold, mass, probs, rec, logdens, order):
    D, c, nm, npr = abi.MANIFOLD_DIM[manifold], int(rec["count"]), len(mass), len(probs)
    lev = np.array(rec["log_level"][:nm])
    return CredibleRegion(np.array(mass, dtype=np.float64), lev, np.exp(lev), np.array(rec["n_inside"][:nm]), np.array(probs, dtype=np.float64),
                          np.array(rec["quant"][:D, :npr]), np.array(rec["mean"][:D]), c, np.array(logdens[:c]), np.array(order[:c]))


def credibility_from_records(qrecs, single):
    if single:
        return Credibility(float(qrecs["mass"][0]), float(qrecs["logdens"][0]), int(qrecs["n_above"][0]))
    return Credibility(np.array(qrecs["mass"]), np.array(qrecs["logdens"]), np.array(qrecs["n_above"]))


def _options(mass, probs):
    mass = np.atleast_1d(np.asarray(mass, dtype=np.float64)).reshape(-1)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    if len(mass) > abi.CRED_MAX or len(probs) > abi.CRED_MAX:
        raise ValueError(f"credible: at most {abi.CRED_MAX} masses and {abi.CRED_MAX} probabilities per call")
    if not np.all((mass > 0) & (mass <= 1)):
        raise ValueError(f"credible: masses lie in (0, 1], got {mass.tolist()}")
    if not np.all((probs >= 0) & (probs <= 1)):
        raise ValueError(f"credible: probabilities lie in [0, 1], got {probs.tolist()}")
    return mass, probs


def query_points(manifold, dims, pts):
    """reference points of one variable -> (q x 3 tangent coordinates, whether one point was given).  A point has D coordinates, or
    one per entry of `dims` (in the order of `dims`); the entries outside `dims` are not read."""
    D = abi.MANIFOLD_DIM[manifold]
    p = np.asarray(pts, dtype=np.float64)
    single = p.ndim <= 1  # (a scalar or a vector: ONE point; several points: q x width)
    cols = list(range(D)) if dims is None else [int(d) - 1 for d in np.atleast_1d(dims)]
    width = p.shape[-1] if p.ndim > 1 else p.size
    p = p.reshape(-1, width)
    out = np.zeros((p.shape[0], abi.MAXD))
    if width == D:
        out[:, :D] = p
    elif width == len(cols):
        out[:, cols] = p
    else:
        raise ValueError(f"credibility: a point has {D} coordinates" + (f" or {len(cols)} (one per entry of dims)" if dims is not None else "")
                         + f", got {width}")
    if not np.all(np.isfinite(out[:, cols])):
        raise ValueError("credibility: a reference point is not finite")
    return out, single


_NO_HOST_ROUTE = "belief overlaps are computed by libnbp"  # (the wording these refusals have always had; beliefquery._backend)


def region_columns(fg, labels, dims, place):
    """(slots, manifolds, masks) of run_credible for variable labels; place: label -> slot"""
    mans = [_manifold(fg.getVariable(v).varType) for v in labels]
    return [place[v] for v in labels], mans, [dims_mask(m, dims) for m in mans]


def credibleRegionAll(fg, labels=None, mass=MASS, probs=PROBS, dims=None, backend=None):
    """The credible regions of the variables' current beliefs -> {label: CredibleRegion} (labels: default every variable, in
    natural order).  mass: up to 8 masses in (0, 1]; probs: up to 8 probabilities in [0, 1]; dims: the 1-BASED coordinates the
    density is taken on (None: all).  The beliefs go to slots once and ONE run_credible serves them all."""
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    mass, probs = _options(mass, probs)
    if not labels:
        return {}
    cols = region_columns(fg, labels, dims, {v: i for i, v in enumerate(labels)})
    with _staged(fg, labels, backend, "run_credible", _bw, _NO_HOST_ROUTE) as (be, _):
        recs, ld, od, _, _ = be.run_credible(*cols, mass, probs)
    return {v: region_from_records(m, mass, probs, recs[i], ld[i], od[i]) for i, (v, m) in enumerate(zip(labels, cols[1]))}


def credibleRegion(fg, label, mass=MASS, probs=PROBS, dims=None, backend=None):
    """The credible regions of one variable's current belief -> CredibleRegion (see credibleRegionAll)"""
    return credibleRegionAll(fg, [label], mass, probs, dims, backend)[label]


def credibility(fg, points, dims=None, backend=None):
    """The credibility of reference points under the variables' current beliefs: points = {label: point or points} (tangent
    coordinates: D per point, or one per entry of `dims`) -> {label: Credibility(mass, logdens, n_above)} -- e.g. the ground truth of
    every variable, and `coverage` of the result is the calibration table.  The beliefs go to slots once and ONE run_credible serves
    every point of every variable."""
    labels = list(points)
    if not labels:
        return {}
    cols = region_columns(fg, labels, dims, {v: i for i, v in enumerate(labels)})
    packed = [query_points(m, dims, points[v]) for v, m in zip(labels, cols[1])]
    with _staged(fg, labels, backend, "run_credible", _bw, _NO_HOST_ROUTE) as (be, _):
        _, _, _, qrecs, first = be.run_credible(*cols, (), (), [q for q, _ in packed], logdens=False, order=False)
    return {v: credibility_from_records(qrecs[first[i]:first[i + 1]], packed[i][1]) for i, v in enumerate(labels)}


def belief_credible(manifold, pts, bw, mass=MASS, probs=PROBS, dims=None, backend=None):
    """`Belief.credible`: the credible regions of a belief held on the host (nbp_kde_credible, through slot 0)"""
    mass, probs = _options(mass, probs)
    with _backend(backend, len(pts), 1, "kde_credible", _NO_HOST_ROUTE) as be:
        rec, ld, od, _ = be.kde_credible(manifold, pts, _bw(manifold, bw), dims_mask(manifold, dims), mass, probs)
    return region_from_records(manifold, mass, probs, rec, ld, od)


def belief_credibility(manifold, pts, bw, points, dims=None, backend=None):
    """`Belief.credibility`: the credibility of reference points under a belief held on the host (nbp_kde_credible)"""
    Q, single = query_points(manifold, dims, points)
    with _backend(backend, len(pts), 1, "kde_credible", _NO_HOST_ROUTE) as be:
        _, _, _, qrecs = be.kde_credible(manifold, pts, _bw(manifold, bw), dims_mask(manifold, dims), (), (), Q, logdens=False, order=False)
    return credibility_from_records(qrecs, single)
