"""Belief queries: the density of a belief at query points, and the distance between two beliefs.

  getBelief(fg, :x0)([l0])              the call the reference's multi-modal tests are made of (test/testMultiHypo3Door.jl:96-165)
  mmd(p1, p2, varType; bw = [0.001])    src/services/SolverUtilities.jl:25-47
  isapprox(p1, p2; atol = 1e-6)         src/services/CompareUtils.jl:11-18 (here: isapproxBeliefs)
  mmdSolveKey                           src/services/AnalysisTools.jl:164-176 (here: mmdVariables, over two graphs)

The definitions, for a belief of c points x_j on a manifold of dimension D with bandwidth h, in tangent coordinates
at the identity (SE(2): x, y, theta):

  density  p(q) = 1 / (c prod_d sqrt(2 pi) h_d) * sum_{j < c} exp(-1/2 sum_d (delta_d(q, x_j) / h_d)^2), delta wrapped to [-pi, pi)
           on circular coordinates (Circular, the heading of SE(2)).  The kernel of the PPE's p_i (ppe.py) with the normalisation
           added: exact on Euclidean coordinates; on a circular coordinate the mass a kernel has beyond +-pi is lost.  All D
           coordinates enter: partial beliefs are not treated specially.  A bandwidth entry that is not positive and finite:
           every density is NaN.
  mmd      k(p, q) = exp(-sigma d(p, q)^2), d^2 = sum_d w_d delta_d^2 (circular coordinates wrapped; w_d = 1 everywhere, the heading
           of SE(2) included: SE2_HEADING_WEIGHT), S_xy = sum_i sum_j k(x_i, y_j); for a of n points and b of m points
           mmd = Saa / (n n) + Sbb / (m m) - 2 Sab / (n m), evaluated as written, no clamp at zero.  sigma is the reference's
           bw[1]; the beliefs' own bandwidths play no part.

Both are DEFINED here and are not pinned against the Julia packages: KernelDensityEstimate.jl's evaluation and
ApproxManifoldProducts' `mmd` / `ker` are not part of the reference's source tree; the form of `ker` is restated from memory,
and Manifolds.jl's metric on SE(2) would weigh the squared heading by 2 where this weighs it by 1.

On a HIP backend both are one kernel launch for any number of resident beliefs (`HipBackend.run_evaluate`, `run_mmd`;
csrc/nbp_query.h).  `density_numpy` and `mmd_numpy` restate the definitions on the host and serve wherever no such backend is at
hand (the CPU oracle has no such entry point)."""
import math
from contextlib import closing, contextmanager, nullcontext

import numpy as np

from . import abi
from .ppe import _circular, _natural, ppe_coords  # noqa: F401  (ppe_coords: host points -> tangent coordinates)

SE2_HEADING_WEIGHT = 1.0  # NBP_MMD_SE2_HEADING_WEIGHT of csrc/nbp_query.h
_SQRT_2PI = math.sqrt(2.0 * math.pi)
_FSUM_ROW = 2048  # mmd_numpy: rows up to this length are added with math.fsum


def _wrap(a):
    """to [-pi, pi), the identity on that interval (as nbpm_wrap_pi of include/nbp_math.h is)"""
    a = np.asarray(a, dtype=np.float64)
    return np.where((a >= -np.pi) & (a < np.pi), a, (a + np.pi) % (2 * np.pi) - np.pi)


def _manifold(varType):
    return int(varType) if isinstance(varType, (int, np.integer)) else varType.manifold


def _queries(manifold, q):
    """tangent coordinates of query points: q x D from (q x D), or one point from a vector of D"""
    q = np.asarray(q, dtype=np.float64)
    return q.reshape(-1, abi.MANIFOLD_DIM[manifold])


def density_numpy(manifold, X, bw, Q):
    """the density of the definition: X (c x D) the belief's tangent coordinates, bw its bandwidth, Q (q x D) the queries ->
    q densities.  The sum over j is exact (math.fsum)."""
    D = abi.MANIFOLD_DIM[manifold]
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    Q = _queries(manifold, Q)
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)[:D]
    if len(bw) < D or not np.all(np.isfinite(bw) & (bw > 0)):
        return np.full(Q.shape[0], np.nan)
    circ = _circular(manifold)
    norm = float(X.shape[0])
    for d in range(D):
        norm *= _SQRT_2PI * bw[d]
    out = np.zeros(Q.shape[0])
    for i in range(Q.shape[0]):
        e = np.zeros(X.shape[0])
        for d in range(D):
            dl = Q[i, d] - X[:, d]
            if circ[d]:
                dl = _wrap(dl)
            e += (dl / bw[d]) ** 2
        out[i] = math.fsum(np.exp(-0.5 * e).tolist()) / norm
    return out


def _kernel_sum(manifold, A, B, sigma):
    """S_ab = sum_i sum_j exp(-sigma d(a_i, b_j)^2)"""
    circ = _circular(manifold)
    rows = []
    step = max(1, (1 << 21) // max(B.shape[0], 1))
    for i0 in range(0, A.shape[0], step):
        e = np.zeros((min(step, A.shape[0] - i0), B.shape[0]))
        for d in range(A.shape[1]):
            dl = A[i0:i0 + step, d, None] - B[None, :, d]
            if circ[d]:
                dl = _wrap(dl)
            w = SE2_HEADING_WEIGHT if (manifold == abi.SE2 and d == 2) else 1.0
            e += w * dl * dl
        k = np.exp(-sigma * e)
        if B.shape[0] <= _FSUM_ROW:
            rows += [math.fsum(r) for r in k.tolist()]
        else:
            rows += k.sum(axis=1).tolist()
    return math.fsum(rows)


def mmd_numpy(manifold, A, B, sigma=0.001):
    """the mmd of the definition: A (n x D), B (m x D) tangent coordinates.  The three pair sums are exact (math.fsum) for beliefs
    of up to 2048 points -- every belief the library holds; beyond, a row is added pairwise by numpy (relative error of a row
    <= log2(m) 2^-53) and the rows by math.fsum."""
    D = abi.MANIFOLD_DIM[manifold]
    A = np.asarray(A, dtype=np.float64).reshape(-1, D)
    B = np.asarray(B, dtype=np.float64).reshape(-1, D)
    n, m = float(A.shape[0]), float(B.shape[0])
    saa, sbb, sab = _kernel_sum(manifold, A, A, sigma), _kernel_sum(manifold, B, B, sigma), _kernel_sum(manifold, A, B, sigma)
    return saa / (n * n) + sbb / (m * m) - 2 * sab / (n * m)


@contextmanager
def _backend(backend, N, n_slots, method, required=None):
    """with _backend(...) as be: the backend a query runs on -- `backend` (class, factory or instance) where it has `method`, else
    None: the numpy route.  One made here is closed on the way out, however the block ends.  required: the family has no host route
    -- None means HipBackend, and a backend without `method` is a ValueError that opens with this text"""
    from .solver import _make_backend
    be, own = (None, False) if backend is None and not required else _make_backend(backend, max(int(N), 8), n_slots)
    with closing(be) if own else nullcontext():
        if getattr(be, method, None) is not None:
            yield be
        elif required:
            raise ValueError(f"{required}: the backend has no {method}")
        else:
            yield None


def _bw(manifold, bw):
    """a bandwidth of D entries: what a slot takes (entries a short bandwidth lacks are 0: unusable where the mask needs them)"""
    D = abi.MANIFOLD_DIM[manifold]
    out = np.zeros(D)
    bw = np.asarray([] if bw is None else bw, dtype=np.float64).reshape(-1)[:D]
    out[:len(bw)] = bw
    return out


def _bw_ones(manifold, bw):
    """for the queries a bandwidth plays no part in: the slot of a belief that has none carries ones"""
    return bw if bw is not None else np.ones(abi.MANIFOLD_DIM[manifold])


@contextmanager
def _staged(fg, labels, backend, method, bw=lambda manifold, bw: bw, required=None):
    """with _staged(...) as (be, place): `_backend`, with the beliefs of the variables `labels` written to slots 0 .. L-1 by ONE
    beliefs_write where there is a backend; place: label -> slot.  bw(manifold, v.bw): the bandwidth a slot is given (default: as
    stored; `_bw_ones`; `_bw`)"""
    vs = [fg.getVariable(v) for v in labels]
    mans = [_manifold(v.varType) for v in vs]
    with _backend(backend, max([len(v.val) for v in vs] + [1]), max(len(vs), 1), method, required) as be:
        if be is not None and vs:
            be.beliefs_write(list(range(len(vs))), mans, [(v.val, bw(m, v.bw), None) for v, m in zip(vs, mans)])
        yield be, {v: i for i, v in enumerate(labels)}


class Belief:
    """What getBelief returns: the belief's manifold, points (host form, N x P) and bandwidth; calling it evaluates the density"""

    def __init__(self, manifold, pts, bw):
        self.manifold = _manifold(manifold)
        self.pts = np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[self.manifold])
        self.bw = np.asarray(bw, dtype=np.float64).reshape(-1)

    def __call__(self, pts, backend=None):
        """belief(pts): densities at host points (q x P), or at one point (a vector of P, or a scalar on a 1-D manifold).
        `backend`: a HIP backend (class, factory or instance: nbp_kde_evaluate, through slot 0); anything without that entry
        point, or None: numpy."""
        Q = ppe_coords(self.manifold, np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[self.manifold]))
        with _backend(backend, len(self.pts), 1, "kde_evaluate") as be:
            if be is not None:
                return be.kde_evaluate(self.manifold, self.pts, self.bw, Q)
            return density_numpy(self.manifold, ppe_coords(self.manifold, self.pts), self.bw, Q)

    def marginal(self, dims):
        """belief.marginal(dims): the marginal density on the 1-BASED coordinates `dims` (marginal.py) -- callable at host points,
        with a `.grid(n, extent=None, margin=4.0, backend=None)` method; a partial belief has one on its partial coordinates"""
        from .marginal import Marginal
        return Marginal(self, dims)

    def modes(self, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE, backend=None):
        """belief.modes(): the modes of the belief's KDE by mean-shift from every one of its points (modes.py) -> BeliefModes;
        `backend` as in `__call__` (nbp_kde_modes, through slot 0)"""
        from .modes import belief_modes
        return belief_modes(self.manifold, self.pts, self.bw, bwScale, tol, maxIter, merge, backend)

    def credible(self, mass=(0.5, 0.9, 0.95), probs=(0.025, 0.25, 0.5, 0.75, 0.975), dims=None, backend=None):
        """belief.credible(): the levels of the belief's highest-density regions at `mass` and the quantiles of its coordinates at
        `probs` (credible.py) -> CredibleRegion; dims: the 1-BASED coordinates the density is taken on (None: all); computed by
        libnbp (nbp_kde_credible, through slot 0; backend None: HipBackend)"""
        from .credible import belief_credible
        return belief_credible(self.manifold, self.pts, self.bw, mass, probs, dims, backend)

    def mixture(self, maxComponents=abi.MIX_MAX, bwScale=abi.MODES_BW_SCALE, tol=abi.MIX_TOL, maxIter=abi.MIX_MAX_ITER, backend=None):
        """belief.mixture(): the belief as a Gaussian mixture of at most `maxComponents` components (mixture.py) -> BeliefMixture,
        whose `asPrior(varType)` goes back into a graph; computed by libnbp on a HIP `backend` (nbp_kde_modes and nbp_kde_mixture,
        through slot 0), by numpy otherwise"""
        from .mixture import belief_mixture
        return belief_mixture(self.manifold, self.pts, self.bw, maxComponents, bwScale, tol, maxIter, backend)

    def credibility(self, pts, dims=None, backend=None):
        """belief.credibility(pts): the mass of the smallest highest-density region that still contains each reference point
        (tangent coordinates: one point, or q x D) -> Credibility(mass, logdens, n_above); `dims` and `backend` as in `credible`"""
        from .credible import belief_credibility
        return belief_credibility(self.manifold, self.pts, self.bw, pts, dims, backend)


def getBelief(fg, label):
    """getBelief(dfg, label): the variable's current belief, callable at query points"""
    v = fg.getVariable(label)
    return Belief(v.varType.manifold, v.val, v.bw)


def _points(p):
    return p.pts if isinstance(p, Belief) else p


def mmd(p1, p2, varType, bw=(0.001,), backend=None):
    """mmd(p1, p2, varType; bw): p1, p2 host points (N x P) or beliefs; varType a variable type (or a manifold constant).
    `backend` as in Belief.__call__ (nbp_kde_mmd, through slots 0 and 1)."""
    man = _manifold(varType)
    a = np.asarray(_points(p1), dtype=np.float64).reshape(-1, abi.MANIFOLD_P[man])
    b = np.asarray(_points(p2), dtype=np.float64).reshape(-1, abi.MANIFOLD_P[man])
    sigma = float(bw[0])
    with _backend(backend, max(len(a), len(b)), 2, "kde_mmd") as be:
        if be is not None:
            return be.kde_mmd(man, a, b, sigma)
        return mmd_numpy(man, ppe_coords(man, a), ppe_coords(man, b), sigma)


def isapproxBeliefs(p1, p2, varType, atol=1e-6, backend=None):
    """isapprox(p1, p2; atol) on beliefs: mmd(p1, p2) < atol (CompareUtils.jl:11-18)"""
    return bool(mmd(p1, p2, varType, backend=backend) < atol)


def mmdVariables(fgA, fgB, labels=None, bw=(0.001,), backend=None):
    """the mmd between the beliefs two graphs hold of the same variables (labels: default every variable of fgA, in natural
    order) -> (labels, values).  On a HIP backend both graphs' beliefs are written to slots (A: 0 .. L-1, B: L .. 2L-1) and ONE
    run_mmd compares them all; otherwise numpy."""
    labels = sorted(fgA.ls(), key=_natural) if labels is None else list(labels)
    L = len(labels)
    va, vb = [fgA.getVariable(v) for v in labels], [fgB.getVariable(v) for v in labels]
    mans = [v.varType.manifold for v in va]
    sigma = float(bw[0])
    if L == 0:
        return labels, np.zeros(0)
    with _backend(backend, max(len(v.val) for v in va + vb), 2 * L, "run_mmd") as be:
        if be is not None:
            be.beliefs_write(list(range(2 * L)), mans + mans, [(v.val, v.bw, None) for v in va + vb])
            return labels, be.run_mmd(list(range(L)), list(range(L, 2 * L)), mans, sigma)
        return labels, np.array([mmd_numpy(m, ppe_coords(m, a.val), ppe_coords(m, b.val), sigma) for m, a, b in zip(mans, va, vb)])
