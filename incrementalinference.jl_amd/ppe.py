"""Point estimates of a belief: the mirror of the reference's PPE names.

  calcPPE                          src/services/FGOSUtils.jl:237-275
  setPPE / getPPE                  the `setPPE!` at the end of every setValKDE! (src/services/FactorGraph.jl:200-213)
  getPPESuggested / Mean / Max, getPPESuggestedAll   src/services/FGOSUtils.jl:396-414

The definition, for a belief of c points x[i] on a manifold of dimension D with bandwidth h:

  mean[d]    mean(M, pts, GeodesicInterpolation()) of coordinate d: the running geodesic mean, point by point
  p_i        sum_{j < c} exp(-1/2 sum_{d < D} (delta_d(i, j) / h_d)^2), delta wrapped to [-pi, pi) on circular coordinates
             (Circular, the heading of SE(2)); the self term included, no normalisation, j = 0 .. c - 1 in that order
  max_index  the smallest i whose p_i is the greatest (Julia's argmax);  max = that point's coordinates
  suggested  = mean, as calcPPE sets it (FGOSUtils.jl:268-274)
  a bandwidth entry that is not a positive finite number: max = NaN, max_index = -1, the mean still stands

`max` is the mode of the joint KDE AMONG THE BELIEF'S OWN POINTS.  It stands in for KernelDensityEstimate.jl's getKDEMax,
which is not part of the reference's source tree, and is not pinned against that package; `suggested` and `mean`
-- what the reference's tests read -- do not depend on it.

On a HIP backend the estimate is one kernel launch for any number of resident beliefs (`HipBackend.run_ppe`, nbp_ppe.h);
`ppe_numpy` restates the definition on the host and serves wherever no such backend is at hand (the CPU oracle has no PPE
entry point).  All estimates are tangent coordinates at the identity (SE(2): x, y, theta)."""
import re
from dataclasses import dataclass

import numpy as np

from . import abi


@dataclass
class MeanMaxPPE:
    """MeanMaxPPE of DistributedFactorGraphs.jl: `suggested`, `max`, `mean`, D coordinates each.  `max_index` (not a field of
    the reference's type) names the point of the belief that `max` is; -1 when the bandwidth admits no density."""
    suggested: np.ndarray
    max: np.ndarray
    mean: np.ndarray
    max_index: int = -1


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def _circular(manifold):
    return [(manifold == abi.CIRCULAR and d == 0) or (manifold == abi.SE2 and d == 2) for d in range(abi.MANIFOLD_DIM[manifold])]


def ppe_coords(manifold, pts):
    """host points (N x P) -> tangent coordinates (N x D)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[manifold])
    if manifold == abi.SE2:
        return np.stack([pts[:, 0], pts[:, 1], np.arctan2(pts[:, 3], pts[:, 2])], axis=1)
    return pts


def mean_geodesic_walk(x, circ):
    """the running geodesic mean of one coordinate, point by point (Manifolds.jl's GeodesicInterpolation)"""
    m = float(x[0])
    for i in range(1, len(x)):
        dl = float(x[i]) - m
        if circ:
            dl = _wrap(dl)
        m = m + dl / (i + 1)
        if circ:
            m = _wrap(m)
    return m


def kde_density(manifold, X, bw):
    """p_i of the definition, for tangent coordinates X (c x D): the sum over j runs in the order j = 0 .. c - 1"""
    X, bw = np.asarray(X, dtype=np.float64), np.asarray(bw, dtype=np.float64)
    circ = _circular(manifold)
    p = np.zeros(X.shape[0])
    for j in range(X.shape[0]):
        q = np.zeros(X.shape[0])
        for d in range(X.shape[1]):
            dl = X[:, d] - X[j, d]
            if circ[d]:
                dl = _wrap(dl)
            q += (dl / bw[d]) ** 2
        p += np.exp(-0.5 * q)
    return p


def ppe_numpy(manifold, pts, bw):
    """the definition on the host -> (mean[D], max[D], max_index)"""
    X = ppe_coords(manifold, pts)
    D = abi.MANIFOLD_DIM[manifold]
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)[:D]
    circ = _circular(manifold)
    mean = np.array([mean_geodesic_walk(X[:, d], circ[d]) for d in range(D)])
    if len(bw) < D or not np.all(np.isfinite(bw) & (bw > 0)):
        return mean, np.full(D, np.nan), -1
    i = int(np.argmax(kde_density(manifold, X, bw)))  # the first of equals, like Julia's argmax
    return mean, X[i].copy(), i


def calcPPE(fg, label, backend=None):
    """calcPPE(dfg, label) -> MeanMaxPPE of the variable's current belief.  `backend`: a HIP backend (class, factory or
    instance: the estimate is computed on the device, nbp_kde_ppe); anything without a PPE entry point, or None: numpy."""
    v = fg.getVariable(label)
    man = v.varType.manifold
    from .beliefquery import _backend  # (beliefquery imports this module)
    with _backend(backend, len(v.val), 1, "kde_ppe") as be:
        mean, mx, idx = be.kde_ppe(man, v.val, v.bw) if be is not None else ppe_numpy(man, v.val, v.bw)
    return MeanMaxPPE(mean.copy(), mx, mean, int(idx))


def setPPE(fg, label, ppe=None):
    """setPPE!(dfg, label, ppe): store `ppe`, or the estimate of the current belief, with the variable"""
    v = fg.getVariable(label)
    v.ppe = ppe if ppe is not None else calcPPE(fg, label)
    return v.ppe


def getPPE(fg, label):
    """getPPE(dfg, label): the stored estimate; computed now when the belief changed since (setValKDE drops it)"""
    v = fg.getVariable(label)
    return v.ppe if v.ppe is not None else setPPE(fg, label)


def getPPESuggested(fg, label):
    return getPPE(fg, label).suggested


def getPPEMean(fg, label):
    return getPPE(fg, label).mean


def getPPEMax(fg, label):
    return getPPE(fg, label).max


def _natural(label):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", label)]


def getPPESuggestedAll(fg):
    """-> (labels in natural order, one row of suggested coordinates per variable, zero-padded to the widest)"""
    labels = sorted(fg.ls(), key=_natural)
    sug = [getPPE(fg, v).suggested for v in labels]
    out = np.zeros((len(labels), max((len(s) for s in sug), default=0)))
    for i, s in enumerate(sug):
        out[i, :len(s)] = s
    return labels, out
