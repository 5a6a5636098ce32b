"""Belief overlaps: which variables lie near a location, how much two beliefs overlap, and which beliefs of a graph overlap at all.

  findVariablesNear(dfg, loc, regexFilter; number)   src/services/FGOSUtils.jl:425-437 (exported, src/ExportAPI.jl:308): the
                                                     variables ranked by the distance of their point estimates to `loc`
  findBeliefsNear, beliefOverlap, overlapVariables, findOverlaps      this library's own, belief-aware forms

The reference's primitive ranks by point estimates, and the posteriors this solver exists for make that wrong: the mean of a
two-door belief lies between the doors, near neither.  `findBeliefsNear` ranks by the marginal density at `loc` instead, and the
overlap coefficient says how much two beliefs have in common ("Belief overlaps"; defined here, unpinned: DESIGN.md 8).
Belief a: n points, bandwidth h_a, coordinates K_a; belief b: m points, h_b, K_b; the coordinates in ascending order, position k
of a against position k of b (ADMISSIBLE: the same number of positions D_K, each of the same kind, Euclidean or circular):

  s_k     h_a,k^2 + h_b,k^2;  r_k = 1 / s_k
  e_ij    -1/2 sum_k delta_k(a_i, b_j)^2 r_k, delta = a - b wrapped to [-pi, pi) on circular positions
  L_ab    ((M + log sum_ij exp(e_ij - M)) - log(n m)) - sum_k 1/2 log(2 pi s_k), M = max e_ij, a term below exp(-700) dropped: the
          logarithm of the integral of the product of the two marginal KDEs (exact on Euclidean coordinates; on circular ones the
          mass beyond +-pi is not wrapped back), finite where every density underflows
  logc    L_ab - 1/2 (L_aa + L_bb);  c = exp(logc): 1 for equal beliefs, <= 1 on Euclidean coordinates (Cauchy-Schwarz; not
          guaranteed on circular ones); a bit-identical copy gives logc == 0.0 exactly.  A bandwidth entry in K that is not positive
          and finite: NaN.

  search  every belief has a box [lo_k, hi_k] (exact minimum and maximum of its points per position); pair (i, j) is skipped iff on
          some Euclidean position gap = max(lo_i - hi_j, lo_j - hi_i) > 0 and gap^2 > reach^2 (h_i^2 + h_j^2).  A skipped pair has
          c <= sqrt(n m) exp(-reach^2 / 2); options with log(minCoeff) < log(N) - reach^2 / 2 + 1 are refused, so the search equals
          brute force.  Circular positions never prune.

COORDINATES.  `HipBackend.run_overlap` / `run_overlap_search` and the numpy restatements take 0-based bit masks (bit d = coordinate
d); the `dims` of `findBeliefsNear`, `beliefOverlap`, `overlapVariables` and `findOverlaps` count from 1, like `marginalGrid`.

The device computes the overlaps (csrc/nbp_overlap.h): one workgroup per pair, or one per row of the search.  `overlap_numpy` and
`overlap_search_numpy` restate the definitions in the device's summation order for tests and readers; they are never a fallback."""
import math
import re
from collections import namedtuple

import numpy as np

from . import abi
from .beliefquery import Belief, _backend, _bw, _manifold, _staged
from .likelihood import _coords, _wrap, block_sum_numpy, shifted_exp
from .marginal import marginal_density_numpy
from .ppe import _natural, getPPE, ppe_coords

MAXK, REACH, MIN_COEFF, TOPK = abi.OVERLAP_MAXK, abi.OVERLAP_REACH, abi.OVERLAP_MIN_COEFF, abi.OVERLAP_TOPK
_TWO_PI = 6.28318530717958647692  # NBP_TWO_PI of csrc/nbp_device.h

Overlap = namedtuple("Overlap", "coeff logcoeff logcross logself_a logself_b")


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def mask_coords(manifold, mask):
    """the 0-based coordinates of a bit mask in ascending order; ValueError for an empty mask or a coordinate outside the manifold"""
    D, mask = abi.MANIFOLD_DIM[manifold], int(mask)
    if mask == 0:
        raise ValueError("overlap: empty mask")
    if mask < 0 or mask >> D:
        raise ValueError(f"overlap: coordinate outside the manifold (mask {mask}, dimension {D})")
    return [d for d in range(D) if mask >> d & 1]


def mask_kinds(manifold, mask):
    """per masked position whether it is circular"""
    return [(manifold == abi.CIRCULAR and d == 0) or (manifold == abi.SE2 and d == 2) for d in mask_coords(manifold, mask)]


def admissible(manifold_a, mask_a, manifold_b, mask_b):
    return mask_kinds(manifold_a, mask_a) == mask_kinds(manifold_b, mask_b)


def dims_mask(manifold, dims=None):
    """1-BASED coordinates (None: all the manifold has) -> the bit mask"""
    D = abi.MANIFOLD_DIM[manifold]
    if dims is None:
        return (1 << D) - 1
    dims = [int(d) for d in np.atleast_1d(dims)]
    if not dims or len(set(dims)) != len(dims) or min(dims) < 1 or max(dims) > D:
        raise ValueError(f"overlap: distinct 1-based coordinates within 1..{D}, got {dims}")
    return sum(1 << (d - 1) for d in dims)


# ------------------------------------------------------------------------------------------------
# the definition on the host, in the device's order
# ------------------------------------------------------------------------------------------------
def _masked(manifold, pts, bw, mask, T):
    """(points on the masked positions (n x D_K), their bandwidth (D_K) or None when it is unusable, kinds)"""
    cols = mask_coords(manifold, mask)
    X = _coords(manifold, pts, T)[:, cols]
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    h = np.array([bw[d] if d < len(bw) else np.nan for d in cols], dtype=np.float64)
    ok = bool(np.all(np.isfinite(h) & (h > 0)))
    return X, (h.astype(T) if ok else None), mask_kinds(manifold, mask)


def cross_term_numpy(X, hx, Y, hy, kinds, dtype=np.float64):
    """L_xy of the definition in the arithmetic `dtype`: X (n x D_K; the lanes own its rows), Y (m x D_K; walked in order), the
    masked bandwidths, the positions' kinds.  The running sum over j, then block_sum over i: the device's order."""
    T = dtype
    X, Y = np.asarray(X, dtype=T), np.asarray(Y, dtype=T)
    n, m = X.shape[0], Y.shape[0]
    s = [T(hx[k]) * T(hx[k]) + T(hy[k]) * T(hy[k]) for k in range(len(kinds))]
    if not all(np.isfinite(v) and v > 0 for v in s):
        return T(np.nan)
    q = None
    for k, circ in enumerate(kinds):
        d = X[:, None, k] - Y[None, :, k]
        if circ:
            d = _wrap(d, T)
        term = (d * d) * (T(1) / s[k])
        q = term if q is None else q + term
    e = T(-0.5) * q
    M = e.max()
    S = block_sum_numpy(np.cumsum(shifted_exp(e - M, T), axis=1)[:, -1])
    norm = None
    for v in s:
        t = T(0.5) * np.log(T(_TWO_PI) * v)
        norm = t if norm is None else norm + t
    return ((M + np.log(S)) - np.log(T(n) * T(m))) - norm


def overlap_numpy(manifold_a, a, bw_a, mask_a, manifold_b, b, bw_b, mask_b, dtype=np.float64):
    """the pair form of the definition on the host, in the arithmetic `dtype` (np.longdouble: the measure of a case's conditioning)
    and the device's summation order.  a, b: host points (n x P) or tangent coordinates (n x D); masks: 0-based bit masks ->
    (logc, L_ab, L_aa, L_bb); NaN for an unusable bandwidth.  ValueError for an inadmissible pair."""
    T = dtype
    A, ha, ka = _masked(manifold_a, a, bw_a, mask_a, T)
    B, hb, kb = _masked(manifold_b, b, bw_b, mask_b, T)
    if ka != kb:
        raise ValueError("overlap: inadmissible pair: the masked coordinates differ in number or kind")
    if A.shape[0] < 1 or B.shape[0] < 1:
        raise ValueError("overlap: a belief holds at least one point")
    nan = T(np.nan)
    if ha is None or hb is None:
        return nan, nan, nan, nan
    laa, lbb, lab = cross_term_numpy(A, ha, A, ha, ka, T), cross_term_numpy(B, hb, B, hb, ka, T), cross_term_numpy(A, ha, B, hb, ka, T)
    if not (np.isfinite(laa) and np.isfinite(lbb) and np.isfinite(lab)):
        return nan, nan, nan, nan
    return lab - T(0.5) * (laa + lbb), lab, laa, lbb


def check_search_options(topk, min_coeff, reach, N):
    """what nbp_run_overlap_search refuses, as ValueError"""
    if not (reach > 0 and math.isfinite(reach)) or not (min_coeff > 0 and math.isfinite(min_coeff)):
        raise ValueError("overlap search: reach and min_coeff must be positive and finite")
    if not 1 <= int(topk) <= MAXK:
        raise ValueError(f"overlap search: topk outside 1 .. {MAXK}")
    if not math.log(min_coeff) >= math.log(float(N)) - 0.5 * (reach * reach) + 1.0:
        raise ValueError("overlap search: log(min_coeff) must be at least log(N) - reach^2 / 2 + 1 (a skipped pair could pass the threshold)")


def box_skips(lo_i, hi_i, h_i, lo_j, hi_j, h_j, kinds, reach):
    """the box rule of the search, as the device writes it (float64, no square root)"""
    reach2 = np.float64(reach) * np.float64(reach)
    for k, circ in enumerate(kinds):
        if circ:
            continue
        gap = max(np.float64(lo_i[k]) - np.float64(hi_j[k]), np.float64(lo_j[k]) - np.float64(hi_i[k]))
        if gap > 0.0 and gap * gap > reach2 * (np.float64(h_i[k]) * np.float64(h_i[k]) + np.float64(h_j[k]) * np.float64(h_j[k])):
            return True
    return False


def rank_row(cands, topk, logmin):
    """(index, logc) candidates of one row -> (idx[topk], logc[topk], n_found): at or above the threshold, descending logc, ties to
    the lower index; unused entries -1 / -inf"""
    keep = sorted(((j, v) for j, v in cands if v >= logmin), key=lambda t: (-t[1], t[0]))
    idx, val = np.full(topk, -1, dtype=np.int32), np.full(topk, -np.inf)
    for r, (j, v) in enumerate(keep[:topk]):
        idx[r], val[r] = j, v
    return idx, val, len(keep)


def overlap_search_numpy(beliefs, topk=TOPK, min_coeff=MIN_COEFF, reach=REACH, N=None, dtype=np.float64, prune=True):
    """the search of the definition on the host: beliefs = [(manifold, points, bw, mask), ...], mutually admissible; N: the
    particle count the soundness rule is checked with (default: the largest belief).  Brute force over the pairs the box rule
    keeps (prune=False: over all pairs), every pair evaluated once with a = the lower index ->
    (idx[V, topk], logc[V, topk], n_found[V], n_evaluated[V])"""
    V = len(beliefs)
    parts = [_masked(m, p, bw, k, dtype) for m, p, bw, k in beliefs]
    kinds = parts[0][2] if V else []
    for i, p in enumerate(parts):
        if p[2] != kinds:
            raise ValueError(f"overlap search: belief {i} is not admissible against belief 0")
    check_search_options(topk, min_coeff, reach, max([p[0].shape[0] for p in parts], default=1) if N is None else N)
    valid = []
    for X, h, _ in parts:
        ok = h is not None
        if ok:
            s = [h[k] * h[k] + h[k] * h[k] for k in range(len(kinds))]
            ok = all(np.isfinite(v) and v > 0 for v in s)
        valid.append(ok)
    LO = np.array([np.asarray(X, dtype=np.float64).min(axis=0) for X, _, _ in parts]).reshape(V, -1)
    HI = np.array([np.asarray(X, dtype=np.float64).max(axis=0) for X, _, _ in parts]).reshape(V, -1)
    H = np.array([np.asarray(h, dtype=np.float64) if ok else np.full(len(kinds), np.nan) for (_, h, _), ok in zip(parts, valid)]).reshape(V, -1)
    eucl = [k for k, circ in enumerate(kinds) if not circ]
    reach2 = np.float64(reach) * np.float64(reach)
    self_term = [cross_term_numpy(X, h, X, h, kinds, dtype) if ok else None for (X, h, _), ok in zip(parts, valid)]
    cands = [[] for _ in range(V)]
    ok_arr = np.array(valid, dtype=bool)
    for i in range(V - 1):
        if not valid[i]:
            continue
        keep = ok_arr[i + 1:].copy()
        if prune and eucl:  # box_skips, row i against every j > i at once: the same float64 operations element by element
            with np.errstate(invalid="ignore"):
                gap = np.maximum(LO[i, eucl] - HI[i + 1:, eucl], LO[i + 1:, eucl] - HI[i, eucl])
                keep &= ~np.any((gap > 0.0) & (gap * gap > reach2 * (H[i, eucl] * H[i, eucl] + H[i + 1:, eucl] * H[i + 1:, eucl])), axis=1)
        for j in (i + 1 + np.flatnonzero(keep)).tolist():
            lab = cross_term_numpy(parts[i][0], parts[i][1], parts[j][0], parts[j][1], kinds, dtype)
            logc = float(lab - dtype(0.5) * (self_term[i] + self_term[j]))
            cands[i].append((j, logc))
            cands[j].append((i, logc))
    idx, val = np.full((V, topk), -1, dtype=np.int32), np.full((V, topk), -np.inf)
    found, evaluated = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    logmin = math.log(min_coeff)
    for i in range(V):
        if not valid[i]:
            found[i] = -1
            continue
        idx[i], val[i], found[i] = rank_row(cands[i], topk, logmin)
        evaluated[i] = len(cands[i])
    return idx, val, found, evaluated


# ------------------------------------------------------------------------------------------------
# the reference's primitive, and its belief-aware form
# ------------------------------------------------------------------------------------------------
def _filtered(fg, regexFilter):
    labels = sorted(fg.ls(), key=_natural)
    if regexFilter is None:
        return labels
    rx = re.compile(regexFilter) if isinstance(regexFilter, str) else regexFilter
    return [v for v in labels if rx.search(v)]


def findVariablesNear(fg, loc, regexFilter=None, number=3):
    """findVariablesNear(dfg, loc, regexFilter; number) (FGOSUtils.jl:425-437) -> (labels, distances): the `number` variables whose
    suggested point estimates (zero-padded to the widest, as getPPESuggestedAll lays them out) lie nearest to `loc` over the first
    len(loc) coordinates, nearest first.  Host only.  It ranks point estimates: see `findBeliefsNear` for multi-modal beliefs."""
    loc = np.asarray(loc, dtype=np.float64).reshape(-1)
    labels = _filtered(fg, regexFilter)
    sug = [getPPE(fg, v).suggested for v in labels]
    xy = np.zeros((len(labels), max([len(s) for s in sug] + [len(loc)])))
    for i, s in enumerate(sug):
        xy[i, :len(s)] = s
    dist = ((xy[:, :len(loc)] - loc[None, :]) ** 2).sum(axis=1)
    prm = np.argsort(dist, kind="stable")[:number]
    return [labels[i] for i in prm], np.sqrt(dist[prm])


def findBeliefsNear(fg, loc, dims=None, number=3, regexFilter=None, backend=None):
    """The belief-aware form of findVariablesNear -> (labels, densities): the `number` variables whose beliefs put the highest
    marginal density at `loc`, highest first (ties in natural order).  dims: the 1-BASED coordinates `loc` is given on (default: the
    first len(loc)); variables whose manifold lacks one of them are left out.  `backend`: a HIP backend (class, factory or instance:
    the beliefs go to slots 0 .. L-1 and ONE run_evaluate_marginal serves them all); None: numpy (marginal_density_numpy)."""
    loc = np.asarray(loc, dtype=np.float64).reshape(-1)
    dims = tuple(range(1, len(loc) + 1)) if dims is None else tuple(int(d) for d in np.atleast_1d(dims))
    if len(dims) != len(loc) or len(set(dims)) != len(dims) or min(dims) < 1:
        raise ValueError("findBeliefsNear: one distinct 1-based coordinate per entry of loc")
    labels = [v for v in _filtered(fg, regexFilter) if fg.getVariable(v).varType.dim >= max(dims)]
    if not labels:
        return [], np.zeros(0)
    vs = [fg.getVariable(v) for v in labels]
    mans = [_manifold(v.varType) for v in vs]
    Q = np.zeros((1, abi.MAXD))
    for d, x in zip(dims, loc):
        Q[0, d - 1] = x
    with _staged(fg, labels, backend, "run_evaluate_marginal") as (be, _):
        if be is not None:
            got = be.run_evaluate_marginal(list(range(len(vs))), mans, [dims_mask(m, dims) for m in mans], [Q] * len(vs))
            dens = np.array([g[0] for g in got])
        else:
            dens = np.array([marginal_density_numpy(m, ppe_coords(m, v.val), v.bw, [d - 1 for d in dims], Q[:, :abi.MANIFOLD_DIM[m]])[0]
                             for m, v in zip(mans, vs)])
    prm = sorted(range(len(labels)), key=lambda i: (-dens[i] if np.isfinite(dens[i]) else np.inf, i))[:number]
    return [labels[i] for i in prm], dens[prm]


# ------------------------------------------------------------------------------------------------
# overlaps on the device
# ------------------------------------------------------------------------------------------------
_NO_HOST_ROUTE = "belief overlaps are computed by libnbp"  # (`required` of beliefquery._backend: None means HipBackend)


def overlap_from_rec(rec):
    logc = float(rec[0])
    return Overlap(math.exp(logc) if logc == logc else math.nan, logc, float(rec[1]), float(rec[2]), float(rec[3]))


def _belief(p, what):
    if isinstance(p, Belief):
        return p.pts, p.bw
    if isinstance(p, tuple) and len(p) == 2 and p[1] is not None:
        return p
    raise ValueError(f"{what}: an overlap needs the belief's bandwidth: pass a Belief (getBelief) or a (points, bw) pair")


def beliefOverlap(p1, p2, varType, dims=None, backend=None):
    """The overlap of two beliefs -> Overlap(coeff, logcoeff, logcross, logself_a, logself_b).  p1, p2: beliefs (getBelief) or (host
    points N x P, bandwidth) pairs; varType: the variable type (or manifold constant) of both, or a pair of them; dims: the 1-BASED
    coordinates compared (default: all), or a pair of such lists, one per belief.  nbp_kde_overlap, through slots 0 and 1."""
    ta, tb = varType if isinstance(varType, (tuple, list)) else (varType, varType)
    ma, mb = _manifold(ta), _manifold(tb)
    da, db = dims if (dims is not None and len(dims) == 2 and all(hasattr(d, "__len__") for d in dims)) else (dims, dims)
    (a, bw_a), (b, bw_b) = _belief(p1, "beliefOverlap"), _belief(p2, "beliefOverlap")
    ka, kb = dims_mask(ma, da), dims_mask(mb, db)
    if not admissible(ma, ka, mb, kb):
        raise ValueError("beliefOverlap: inadmissible pair: the compared coordinates differ in number or kind")
    a = np.asarray(a, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[ma])
    b = np.asarray(b, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[mb])
    with _backend(backend, max(len(a), len(b)), 2, "kde_overlap", _NO_HOST_ROUTE) as be:
        return overlap_from_rec(be.kde_overlap(ma, a, _bw(ma, bw_a), ka, mb, b, _bw(mb, bw_b), kb))


def pair_columns(fg, pairs, dims, place):
    """the six columns of run_overlap for pairs of variable labels; place: label -> slot"""
    var = fg.getVariable
    cols = [[], [], [], [], [], []]
    for k, (u, v) in enumerate(pairs):
        mu, mv = _manifold(var(u).varType), _manifold(var(v).varType)
        ku, kv = dims_mask(mu, dims), dims_mask(mv, dims)
        if not admissible(mu, ku, mv, kv):
            raise ValueError(f"overlapVariables: pair {k} ({u}, {v}) is inadmissible: the compared coordinates differ in number or kind")
        for c, x in zip(cols, (place[u], place[v], mu, mv, ku, kv)):
            c.append(x)
    return cols


def overlapVariables(fg, pairs, dims=None, backend=None):
    """The overlaps of pairs of variables' current beliefs -> {(label_a, label_b): Overlap}.  dims: the 1-BASED coordinates compared
    (default: all; then the two variables of a pair share a manifold's kinds).  The beliefs go to slots once and ONE run_overlap
    serves every pair."""
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        return {}
    labels = []
    for p in pairs:
        labels += [v for v in p if v not in labels]
    cols = pair_columns(fg, pairs, dims, {v: i for i, v in enumerate(labels)})
    with _staged(fg, labels, backend, "run_overlap", _bw, _NO_HOST_ROUTE) as (be, _):
        recs = be.run_overlap(*cols)
    return {p: overlap_from_rec(r) for p, r in zip(pairs, recs)}


class Overlaps(dict):
    """findOverlaps' result: {label: [(partner label, coeff), ...]} in descending order of the coefficient, at most `number` per
    label; `.logcoeff[label]` the same with log-coefficients, `.n_found[label]` ALL partners at or above the threshold (above
    `number`: the list is truncated; -1: the belief's bandwidth is unusable), `.n_evaluated[label]` the pairs the box rule kept"""

    def __init__(self, labels, idx, logc, found, evaluated):
        super().__init__()
        self.labels = list(labels)
        self.logcoeff, self.n_found, self.n_evaluated = {}, {}, {}
        self.idx, self.logc = np.array(idx), np.array(logc)
        for i, v in enumerate(self.labels):
            row = [(self.labels[j], float(x)) for j, x in zip(self.idx[i], self.logc[i]) if j >= 0]
            self.logcoeff[v] = row
            self[v] = [(u, math.exp(x)) for u, x in row]
            self.n_found[v], self.n_evaluated[v] = int(found[i]), int(evaluated[i])

    def pairs(self):
        """the unique pairs, highest coefficient first (ties in list order) -> [(label_a, label_b, coeff)], label_a before label_b
        in the list: the loop-closure candidates"""
        seen = {}
        for i, v in enumerate(self.labels):
            for j, x in zip(self.idx[i], self.logc[i]):
                if j >= 0:
                    seen[(min(i, int(j)), max(i, int(j)))] = float(x)
        order = sorted(seen.items(), key=lambda t: (-t[1], t[0]))
        return [(self.labels[i], self.labels[j], math.exp(x)) for (i, j), x in order]


def search_columns(fg, labels, dims, place):
    """(slots, manifolds, masks) of run_overlap_search; ValueError where the list is not mutually admissible"""
    mans = [_manifold(fg.getVariable(v).varType) for v in labels]
    masks = [dims_mask(m, dims) for m in mans]
    for v, m, k in zip(labels, mans, masks):
        if not admissible(mans[0], masks[0], m, k):
            raise ValueError(f"findOverlaps: {v} cannot be compared with {labels[0]}: "
                             + ("the variables must share one type (or name the coordinates with dims)" if dims is None
                                else "the compared coordinates differ in kind"))
    return [place[v] for v in labels], mans, masks


def findOverlaps(fg, labels=None, dims=None, number=TOPK, minCoeff=MIN_COEFF, reach=REACH, backend=None):
    """Which beliefs of the graph overlap -> Overlaps.  labels: default every variable, in natural order; dims: the 1-BASED
    coordinates compared (None: all, and the variables must share one type; (1, 2): poses and landmarks mix); number: partners kept
    per label (1 .. 16); minCoeff: the threshold; reach: the box rule's reach in bandwidths.  The beliefs go to slots once and ONE
    run_overlap_search serves every row."""
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    if not labels:
        return Overlaps([], np.zeros((0, number), dtype=np.int32), np.zeros((0, number)), [], [])
    cols = search_columns(fg, labels, dims, {v: i for i, v in enumerate(labels)})
    with _staged(fg, labels, backend, "run_overlap_search", _bw, _NO_HOST_ROUTE) as (be, _):
        check_search_options(number, minCoeff, reach, be.N)
        return Overlaps(labels, *be.run_overlap_search(*cols, number, minCoeff, reach))
