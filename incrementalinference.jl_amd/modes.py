"""Modes of a belief: how many hypotheses it still carries, where they are, and what share of the particles each holds.

The reference answers unimodal questions about a posterior (mean, covariance, the one best point); its multi-modal tests
search densities by hand (test/testMultiHypo3Door.jl:96-165).  This query is DEFINED here and unpinned:
KernelDensityEstimate.jl has no mode finder in the reference's tree, and `getKDEMax` lies outside it.

The definition ("Modes of a belief"), for a belief of c points x_j in tangent coordinates at the identity (SE(2): x,
y, theta in the world frame) with bandwidth h, and the options bw_scale, tol, max_iter, merge; g_d = bw_scale h_d:

  ascent   for every start i < c: y <- x_i, then repeat
             w_j = exp(-1/2 sum_d (delta_d(y, x_j) / g_d)^2),  S = sum_j w_j,  m_d = sum_j w_j delta_d(x_j, y),
             y_d <- y_d + m_d / S
           delta wrapped to [-pi, pi) on circular coordinates, y wrapped likewise; j = 0 .. c - 1 in that order.  A start stops
           after the first iteration with max_d |m_d / S| / g_d <= tol (converged) or after max_iter iterations.
  merging  leader clustering in index order: the lowest unassigned i leads, every unassigned k > i with
           max_d |delta_d(y_k, y_i)| / g_d <= merge joins it
  ranking  by member count, descending; equal counts by the lower leader index
  a mode   the leader's end point, the member count, density = S there / (c prod_d sqrt(2 pi) g_d), the leader's index
  a bandwidth entry h_d (or g_d) that is not positive and finite: no modes, every label -1

The defaults: bw_scale 2, tol 1e-6, max_iter 500, merge 1e-2.  The fitted bandwidth is the leave-one-out one and under-smooths
for mode finding (a 200-point Gaussian cloud in three dimensions splits into several modes at scale 1 and has one at scale 2).
merge < 1000 tol is refused: a stopped start may still sit tol rho / (1 - rho) from its fixed point, rho the contraction rate.

On a HIP backend the whole query is one kernel launch for any number of resident beliefs (`HipBackend.run_modes`,
csrc/nbp_modes.h); `modes_numpy` restates the definition on the host, in the same j order, and serves wherever no such backend is
at hand (the CPU oracle has no such entry point)."""
import math
from dataclasses import dataclass

import numpy as np

from . import abi
from .beliefquery import _backend, _staged, _wrap
from .ppe import _circular, _natural, ppe_coords

MODES_MAX = abi.MODES_MAX
_SQRT_2PI = 2.5066282746310002  # NBP_SQRT_2PI of csrc/nbp_kde.h


@dataclass
class BeliefModes:
    """The modes of one belief, the heaviest first.  K = min(n_modes, 32) of them are described; `labels` (the rank of each
    point's mode; -1: the bandwidth admits no density) may name more."""
    modes: np.ndarray      # K x D, tangent coordinates
    counts: np.ndarray     # K, the points whose ascent ended there
    shares: np.ndarray     # K, counts / c
    density: np.ndarray    # K, the KDE at bandwidth bw_scale * bw at the mode
    leader: np.ndarray     # K, the index of the point whose end point the mode is
    labels: np.ndarray     # c
    iters: np.ndarray      # c
    n_unconverged: int
    n_modes: int           # the true number of modes, also above 32


def check_options(bw_scale, tol, max_iter, merge):
    """the refusals of nbp_run_modes, as ValueErrors"""
    if not (bw_scale > 0 and math.isfinite(bw_scale)):
        raise ValueError("modes: bwScale must be positive and finite")
    if not (tol > 0 and math.isfinite(tol)):
        raise ValueError("modes: tol must be positive and finite")
    if not (merge > 0 and math.isfinite(merge)):
        raise ValueError("modes: merge must be positive and finite")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("modes: maxIter must be an integer >= 1")
    if merge < 1000.0 * tol:
        raise ValueError("modes: merge must be at least 1000 tol")


def _sums(manifold, X, g, Y):
    """S[a] and m[a, D] of the definition at the rows of Y (a x D): the sums over j run in the order j = 0 .. c - 1 (a cumulative
    sum along j is that running sum)"""
    circ = _circular(manifold)
    D = X.shape[1]
    e = None
    for d in range(D):
        dl = Y[:, d, None] - X[None, :, d]
        if circ[d]:
            dl = _wrap(dl)
        dl = dl * (1.0 / g[d])
        e = dl * dl if e is None else e + dl * dl
    w = np.exp(-0.5 * e)
    S = np.cumsum(w, axis=1)[:, -1]
    m = np.empty((Y.shape[0], D))
    for d in range(D):
        dl = X[None, :, d] - Y[:, d, None]
        if circ[d]:
            dl = _wrap(dl)
        m[:, d] = np.cumsum(w * dl, axis=1)[:, -1]
    return S, m


def _reach(manifold, dl, g):
    """max_d |delta_d| / g_d of the rows of dl, wrapped on circular coordinates"""
    dl = np.array(dl, dtype=np.float64, copy=True).reshape(-1, len(g))
    for d, circ in enumerate(_circular(manifold)):
        if circ:
            dl[:, d] = _wrap(dl[:, d])
    return (np.abs(dl) / g[None, :]).max(axis=1)


def mean_shift_step(manifold, X, g, Y):
    """max_d |m_d / S| / g_d at the rows of Y: the length of the next step there (a test asks it of the device's end points)"""
    D = abi.MANIFOLD_DIM[manifold]
    X, Y, g = np.asarray(X, dtype=np.float64).reshape(-1, D), np.asarray(Y, dtype=np.float64).reshape(-1, D), np.asarray(g, dtype=np.float64)
    S, m = _sums(manifold, X, g, Y)
    return (np.abs(m / S[:, None]) / g[None, :]).max(axis=1)


def _empty(D, c):
    z = np.zeros(0)
    return BeliefModes(np.zeros((0, D)), z.astype(np.int32), z, z, z.astype(np.int32), np.full(c, -1, dtype=np.int32),
                       np.zeros(c, dtype=np.int32), 0, 0)


def modes_numpy(manifold, pts, bw, bw_scale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, max_iter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE):
    """the definition on the host: pts host points (c x P), bw the belief's bandwidth -> BeliefModes"""
    check_options(bw_scale, tol, max_iter, merge)
    X = np.ascontiguousarray(ppe_coords(manifold, pts))
    D, c = abi.MANIFOLD_DIM[manifold], X.shape[0]
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)[:D]
    g = bw_scale * bw
    if len(bw) < D or not np.all(np.isfinite(bw) & (bw > 0) & np.isfinite(g) & (g > 0)):
        return _empty(D, c)
    circ = _circular(manifold)
    Y = X.copy()
    iters, conv = np.zeros(c, dtype=np.int32), np.zeros(c, dtype=bool)
    act = np.arange(c)
    while act.size:
        S, m = _sums(manifold, X, g, Y[act])
        step = m / S[:, None]
        y = Y[act] + step
        for d in range(D):
            if circ[d]:
                y[:, d] = _wrap(y[:, d])
        Y[act] = y
        iters[act] += 1
        done = (np.abs(step) / g[None, :]).max(axis=1) <= tol
        conv[act[done]] = True
        act = act[~done & (iters[act] < max_iter)]
    lead = np.full(c, -1, dtype=np.int64)
    for i in range(c):
        if lead[i] >= 0:
            continue
        lead[i] = i
        k = np.nonzero(lead[i + 1:] < 0)[0] + i + 1
        if k.size:
            lead[k[_reach(manifold, Y[k] - Y[i][None, :], g) <= merge]] = i
    leaders, counts = np.unique(lead, return_counts=True)
    order = sorted(range(len(leaders)), key=lambda q: (-counts[q], leaders[q]))
    rank = np.zeros(c, dtype=np.int32)
    rank[leaders[order]] = np.arange(len(order))
    kept = leaders[order][:MODES_MAX]
    S, _ = _sums(manifold, X, g, Y[kept])
    norm = float(c)
    for d in range(D):
        norm *= _SQRT_2PI * g[d]
    cnt = counts[order][:MODES_MAX].astype(np.int32)
    return BeliefModes(Y[kept].copy(), cnt, cnt / float(c), S / norm, kept.astype(np.int32), rank[lead].astype(np.int32), iters,
                       int(c - conv.sum()), len(leaders))


def modes_from_records(manifold, recs, n_modes, labels, iters, n_unconverged, c=None):
    """one belief's row of `HipBackend.run_modes` / the result of `kde_modes` -> BeliefModes; c: the points the belief holds
    (None: as many as carry a label; all rows where the bandwidth admits no density)"""
    D, K = abi.MANIFOLD_DIM[manifold], min(int(n_modes), MODES_MAX)
    if c is None:
        c = int((np.asarray(labels) >= 0).sum()) if n_modes > 0 else len(labels)
    cnt = np.array(recs["count"][:K], dtype=np.int32)
    return BeliefModes(np.array(recs["location"][:K, :D]), cnt, cnt / float(max(c, 1)), np.array(recs["density"][:K]),
                       np.array(recs["leader"][:K], dtype=np.int32), np.array(labels[:c], dtype=np.int32), np.array(iters[:c], dtype=np.int32),
                       int(n_unconverged), int(n_modes))


def _options(bwScale, tol, maxIter, merge):
    check_options(bwScale, tol, maxIter, merge)
    return dict(bw_scale=float(bwScale), tol=float(tol), max_iter=int(maxIter), merge=float(merge))


def belief_modes(manifold, pts, bw, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE,
                 backend=None):
    """the modes of a belief held on the host.  `backend`: a HIP backend (class, factory or instance: nbp_kde_modes, through slot
    0); anything without that entry point, or None: numpy."""
    kw = _options(bwScale, tol, maxIter, merge)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[manifold])
    with _backend(backend, len(pts), 1, "kde_modes") as be:
        if be is not None:
            return modes_from_records(manifold, *be.kde_modes(manifold, pts, bw, **kw), len(pts))
        return modes_numpy(manifold, pts, bw, **kw)


def getBeliefModes(fg, label, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE, backend=None):
    """the modes of the variable's current belief -> BeliefModes.  `backend` as in calcPPE."""
    v = fg.getVariable(label)
    return belief_modes(v.varType.manifold, v.val, v.bw, bwScale, tol, maxIter, merge, backend)


def getBeliefModesAll(fg, labels=None, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE,
                      backend=None):
    """-> {label: BeliefModes} (labels: default every variable, in natural order).  On a HIP backend the beliefs are written to
    slots 0 .. L-1 and ONE run_modes finds the modes of all of them; otherwise numpy."""
    kw = _options(bwScale, tol, maxIter, merge)
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    vs = [fg.getVariable(v) for v in labels]
    if not vs:
        return {}
    mans = [v.varType.manifold for v in vs]
    with _staged(fg, labels, backend, "run_modes") as (be, _):
        if be is None:
            return {l: modes_numpy(m, v.val, v.bw, **kw) for l, m, v in zip(labels, mans, vs)}
        res = be.run_modes(list(range(len(vs))), mans, **kw)
        return {l: modes_from_records(m, *(r[i] for r in res), len(v.val)) for i, (l, m, v) in enumerate(zip(labels, mans, vs))}
