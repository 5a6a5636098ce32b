"""Belief statistics: the spread of a belief, and how far one belief has moved from another.

  calcMeanCovar(vari)                   src/services/VariableStatistics.jl:39-44 (what initParametricFrom! reads,
                                        src/parametric/services/ParametricUtils.jl:884)
  Statistics.cov(vartype, pts)          src/services/VariableStatistics.jl:12-19 (the bands of test/testBasicGraphs.jl:47-307)
  kld(p, q)                             attic/examples/FixedPointIllustrationsSquare.jl:53-62 (a convergence monitor)

The definitions ("Belief statistics"), in tangent coordinates at the identity (Euclid(1-3); the circle; SE(2): x, y,
theta), for a belief of c points x[i] on a manifold of dimension D:

  mean[d]      the geodesic mean of ppe.py (on the device: the bits of run_ppe's mean)
  delta[i][d]  x[i][d] - mean[d], wrapped to [-pi, pi) on circular coordinates
  cov[d][e]    (1 / (c - 1)) sum_i delta[i][d] delta[i][e]; c < 2: NaN (Julia's corrected covariance of one observation), the
               mean still stands.  The bandwidth plays no part.
  SE(2)        the deviations are taken in the world frame about the mean, heading wrapped -- NOT the Lie-algebra coordinates at
               the mean that Manifolds.jl's cov(M, pts; basis) would use.  Manifolds.jl is not part of the reference's tree: this
               is DEFINED here and unpinned.
  l_p(x)       M + log(sum_{j < m} exp(e_j - M)) - log(m prod_d sqrt(2 pi) h_d) for a belief p of m points y_j with bandwidth h,
               e_j = -1/2 sum_d (delta_d(x, y_j) / h_d)^2, M = max_j e_j: the logarithm of the density beliefquery.py defines,
               finite where that density underflows to zero
  kld(a, b)    Eaa - Eab, Eaa = (1 / n) sum_i l_a(a_i) (the self term stays in), Eab = (1 / n) sum_i l_b(a_i); no clamp at zero;
               entropy(a) = -Eaa.  A belief against a bit-identical copy of itself gives exactly 0.0.  A bandwidth entry of either
               belief that is not positive and finite: NaN.  This form is restated from memory of KernelDensityEstimate.jl's
               direct `kld` (not part of the reference's tree) and is unpinned.

On a HIP backend each is one kernel launch for any number of resident beliefs (`HipBackend.run_meancov`, `run_kld`;
csrc/nbp_stats.h).  `meancov_numpy` and `kld_numpy` restate the definitions on the host with exact sums and serve wherever no
such backend is at hand (the CPU oracle has no such entry point)."""
import math

import numpy as np

from . import abi
from .beliefquery import Belief, _backend, _bw_ones, _manifold, _staged, _wrap
from .ppe import _circular, _natural, mean_geodesic_walk, ppe_coords

_LOG_SQRT_2PI_ARG = math.sqrt(2.0 * math.pi)


def meancov_numpy(manifold, pts, mean=None):
    """the definition on the host: pts host points (c x P) -> (mean[D], cov[D, D]).  `mean`: deviations are taken about this
    mean (a test hands in the device's) instead of the geodesic walk's.  The D (D + 1) / 2 sums are exact (math.fsum)."""
    X = ppe_coords(manifold, pts)
    D, c = abi.MANIFOLD_DIM[manifold], X.shape[0]
    circ = _circular(manifold)
    if mean is None:
        mean = np.array([mean_geodesic_walk(X[:, d], circ[d]) for d in range(D)])
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)[:D].copy()
    if c < 2:
        return mean, np.full((D, D), np.nan)
    delta = X - mean[None, :]
    for d in range(D):
        if circ[d]:
            delta[:, d] = _wrap(delta[:, d])  # (the identity on [-pi, pi), as the device's wrap is)
    cov = np.zeros((D, D))
    for d in range(D):
        for e in range(d, D):
            cov[d, e] = cov[e, d] = math.fsum((delta[:, d] * delta[:, e]).tolist()) / (c - 1)
    return mean, cov


def _bandwidth(manifold, bw):
    D = abi.MANIFOLD_DIM[manifold]
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)[:D]
    return bw if len(bw) == D and np.all(np.isfinite(bw) & (bw > 0)) else None


def log_density_numpy(manifold, Y, bw, Q):
    """l_p(x) of the definition at the rows of Q (q x D): Y (m x D) the belief's tangent coordinates, bw its bandwidth (positive
    and finite).  Log-sum-exp with an exact sum (math.fsum)."""
    D, m = abi.MANIFOLD_DIM[manifold], Y.shape[0]
    circ = _circular(manifold)
    norm = float(m)
    for d in range(D):
        norm *= _LOG_SQRT_2PI_ARG * bw[d]
    out = np.zeros(Q.shape[0])
    for i in range(Q.shape[0]):
        q = np.zeros(m)
        for d in range(D):
            dl = Q[i, d] - Y[:, d]
            if circ[d]:
                dl = _wrap(dl)
            q += (dl / bw[d]) ** 2
        e = -0.5 * q
        M = float(e.max())
        out[i] = M + math.log(math.fsum(np.exp(e - M).tolist())) - math.log(norm)
    return out


def kld_terms_numpy(manifold, a, bw_a, b, bw_b):
    """(Eaa, Eab) of the definition: a (n x D), b (m x D) tangent coordinates"""
    D = abi.MANIFOLD_DIM[manifold]
    A = np.asarray(a, dtype=np.float64).reshape(-1, D)
    B = np.asarray(b, dtype=np.float64).reshape(-1, D)
    ha, hb = _bandwidth(manifold, bw_a), _bandwidth(manifold, bw_b)
    if ha is None or hb is None:
        return math.nan, math.nan
    n = A.shape[0]
    return (math.fsum(log_density_numpy(manifold, A, ha, A).tolist()) / n,
            math.fsum(log_density_numpy(manifold, B, hb, A).tolist()) / n)


def kld_numpy(manifold, a, bw_a, b, bw_b):
    """the kld of the definition on the host: a (n x D), b (m x D) tangent coordinates with their bandwidths"""
    eaa, eab = kld_terms_numpy(manifold, a, bw_a, b, bw_b)
    return eaa - eab


def calcMeanCovar(fg, label, backend=None):
    """calcMeanCovar(vari) -> (mu[D], Sigma[D, D]) of the variable's current belief.  `backend`: a HIP backend (class, factory or
    instance: computed on the device, nbp_kde_meancov through slot 0); anything without that entry point, or None: numpy."""
    v = fg.getVariable(label)
    man = v.varType.manifold
    with _backend(backend, len(v.val), 1, "kde_meancov") as be:
        if be is not None:
            return be.kde_meancov(man, v.val)
        return meancov_numpy(man, v.val)


def calcMeanCovarAll(fg, labels=None, backend=None):
    """-> {label: (mu, Sigma)} (labels: default every variable, in natural order).  On a HIP backend the beliefs are written to
    slots 0 .. L-1 and ONE run_meancov computes them all; otherwise numpy."""
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    vs = [fg.getVariable(v) for v in labels]
    if not vs:
        return {}
    mans = [v.varType.manifold for v in vs]
    with _staged(fg, labels, backend, "run_meancov", _bw_ones) as (be, _):
        if be is None:
            return {l: meancov_numpy(m, v.val) for l, m, v in zip(labels, mans, vs)}
        mean, cov = be.run_meancov(list(range(len(vs))), mans)
        dims = [abi.MANIFOLD_DIM[m] for m in mans]
        return {l: (mean[i, :D].copy(), cov[i, :D, :D].copy()) for i, (l, D) in enumerate(zip(labels, dims))}


def _points_bw(p, what):
    pts, bw = (p.pts, p.bw) if isinstance(p, Belief) else (p if isinstance(p, tuple) and len(p) == 2 else (p, None))
    if bw is None or np.size(bw) == 0:
        raise ValueError(f"{what}: a kld needs the belief's bandwidth: pass a Belief (getBelief) or a (points, bw) pair")
    return pts, np.asarray(bw, dtype=np.float64).reshape(-1)


def _kld_terms(p1, p2, varType, backend, what):
    man = _manifold(varType)
    a, bw_a = _points_bw(p1, what)
    b, bw_b = _points_bw(p2, what)
    a = np.asarray(a, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[man])
    b = np.asarray(b, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[man])
    D = abi.MANIFOLD_DIM[man]
    if len(bw_a) < D or len(bw_b) < D:
        raise ValueError(f"{what}: a bandwidth of {D} entries is needed")
    with _backend(backend, max(len(a), len(b)), 2, "kde_kld") as be:
        if be is not None:
            val, tm = be.kde_kld(man, a, bw_a[:D], b, bw_b[:D], terms=True)
            return val, float(tm[0]), float(tm[1])
        eaa, eab = kld_terms_numpy(man, ppe_coords(man, a), bw_a, ppe_coords(man, b), bw_b)
        return eaa - eab, eaa, eab


def kld(p1, p2, varType, backend=None):
    """kld(p1, p2): p1, p2 beliefs (getBelief) or (host points N x P, bandwidth) pairs; varType a variable type (or a manifold
    constant).  ValueError when a bandwidth is missing.  `backend` as in calcMeanCovar (nbp_kde_kld, through slots 0 and 1)."""
    return _kld_terms(p1, p2, varType, backend, "kld")[0]


def entropy(p, varType, backend=None):
    """entropy(p) = -Eaa: minus the mean log-density of the belief at its own points (the self term stays in)"""
    return -_kld_terms(p, p, varType, backend, "entropy")[1]
