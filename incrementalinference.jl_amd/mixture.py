"""Mixture summaries of beliefs: a posterior as K <= 8 Gaussians (weights, means, full covariances), the form in which a belief can
go back into a graph (`BeliefMixture.asPrior`) or leave the library (4 x 10 numbers, not 200 x 6).

The reference has the `Mixture` prior and `manikde!` but no fit from one to the other.  This query is DEFINED here and unpinned
(DESIGN.md 8).

The definition ("Mixture summaries"), for a belief of c points x_i in tangent coordinates at the identity (SE(2): x, y,
theta in the world frame) with bandwidth h, H = diag(h_d^2), delta(x, mu) = x - mu wrapped to [-pi, pi) on circular coordinates.
The belief's KDE is a mixture of c Gaussians N(x_i, H); hierarchical EM on the kernel centres reduces it to K components, each
kernel's width entering in expectation:

  start    every particle carries a label -1 .. 7: r_ik = 1 in the component it names, a particle labelled -1 starts in none; mu_k
           starts at a given location; a component is live when a particle carries its label
  M-step   n_k = sum_i r_ik; a live component with n_k < 0.5 is dropped for good; w_k = n_k / sum_l n_l over the live ones;
           mu_k <- wrap(mu_k + sum_i r_ik delta(x_i, mu_k) / n_k); Sigma_k = sum_i r_ik delta_i delta_i^T / n_k + H about the new mean
  E-step   l_ik = log w_k + log N(delta(x_i, mu_k); 0, Sigma_k) - tr(Sigma_k^-1 H) / 2; lse_i = logsumexp_k l_ik (two passes, k
           ascending); r_ik = exp(l_ik - lse_i); J = (1 / c) sum_i lse_i
  stop     after the E-step of iteration t >= 2 when J_t - J_(t-1) <= tol, or after max_iter iterations; tol = 0: max_iter iterations
  result   the live components by weight descending (ties: the lower starting index); count_k = the particles whose greatest r is
           r_ik; labels = the rank of that component
  a bandwidth entry that is not positive and finite, or no label >= 0: no components, every number NaN, every label -1

This is a proper EM on J: the trace term is E_{x ~ N(x_i, H)}[log N(x; mu, Sigma)] - log N(x_i; mu, Sigma), and maximising the bound
over Sigma_k gives exactly "weighted scatter + H".  On Euclidean manifolds J never decreases; Sigma_k >= H, so no component is ever
singular.

The starting labels and means are the modes of the belief (modes.py): the `maxComponents` most populous ones, the particles of the
rest labelled -1.  K is the number of modes, capped; it is not chosen by a criterion and no component is ever split.

On a HIP backend the whole EM of any number of resident beliefs is one kernel launch (`HipBackend.run_mixture`,
csrc/nbp_mixture.h); `mixture_numpy` restates the definition on the host in the device's order of operations and serves wherever no
such backend is at hand."""
import math
from dataclasses import dataclass

import numpy as np

from . import abi
from .beliefquery import _backend, _staged
from .likelihood import _wrap
from .modes import BeliefModes, _options as _mode_options, modes_from_records, modes_numpy
from .ppe import _circular, _natural, ppe_coords

MIX_MAX = abi.MIX_MAX
_LOG_2PI = 1.8378770664093453  # NBP_MIX_LOG_2PI of csrc/nbp_mixture.h


@dataclass
class BeliefMixture:
    """One belief as a Gaussian mixture, the heaviest component first (tangent coordinates at the identity)."""
    manifold: int
    weights: np.ndarray    # K
    means: np.ndarray      # K x D
    covs: np.ndarray       # K x D x D
    counts: np.ndarray     # K, the particles whose greatest responsibility is this component's
    labels: np.ndarray     # c, the rank of each particle's component (-1: there is no fit)
    objective: float       # J
    iters: int
    converged: bool
    n_dropped: int
    modes: BeliefModes = None  # what the fit started from

    @property
    def n_comp(self):
        return len(self.weights)

    def components(self):
        """[(w_k, mu_k, L_k)], L_k the lower Cholesky factor of Sigma_k: what a `Mixture` prior's `components()` hold"""
        return [(float(w), mu.copy(), np.linalg.cholesky(S)) for w, mu, S in zip(self.weights, self.means, self.covs)]

    def asPrior(self, varType):
        """the mixture as a prior factor on a variable of `varType`: Euclid(1-3) `Mixture(Prior, [MvNormal(mu_k, Sigma_k)], w)`; the
        circle `Mixture(PriorCircular, [Normal(mu_k, sqrt(Sigma_k))], w)`; SE(2) `Mixture(ManifoldPrior(0, .), [MvNormal(mu_k,
        Sigma_k)], w)`.  The prior kernel forms wrap(mean + L n) in these same world-frame coordinates (include/nbp.h, nbp_prior_desc),
        so nothing changes frame.  More than NBP_MAXC = 4 components: ValueError."""
        from . import factorgraph as F
        if varType.manifold != self.manifold:
            raise ValueError(f"asPrior: the mixture lives on manifold {self.manifold}, the variable type on {varType.manifold}")
        if self.n_comp < 1:
            raise ValueError("asPrior: the mixture has no components")
        if self.n_comp > abi.MAXC:
            raise ValueError(f"asPrior: a Mixture prior holds at most {abi.MAXC} components and this fit has {self.n_comp}: "
                             f"fit with maxComponents <= {abi.MAXC}")
        if self.manifold == abi.CIRCULAR:
            comps = [F.Normal(float(mu[0]), math.sqrt(float(S[0, 0]))) for mu, S in zip(self.means, self.covs)]
            return F.Mixture(F.PriorCircular, comps, self.weights)
        comps = [F.MvNormal(mu.copy(), S.copy()) for mu, S in zip(self.means, self.covs)]
        if self.manifold == abi.SE2:
            return F.Mixture(F.ManifoldPrior(np.zeros(3), comps[0]), comps, self.weights)
        return F.Mixture(F.Prior, comps, self.weights)

    def logdensity(self, pts):
        """log sum_k w_k N(delta(x, mu_k); 0, Sigma_k) at host points (q x P, or one point) -> q values; host only"""
        D = abi.MANIFOLD_DIM[self.manifold]
        Q = ppe_coords(self.manifold, np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[self.manifold]))
        if self.n_comp < 1:
            return np.full(len(Q), np.nan)
        circ = _circular(self.manifold)
        terms = []
        for w, mu, S in zip(self.weights, self.means, self.covs):
            dl = Q - mu[None, :]
            for d in range(D):
                if circ[d]:
                    dl[:, d] = _wrap(dl[:, d], np.float64)
            L = np.linalg.cholesky(S)
            z = np.linalg.solve(L, dl.T)
            terms.append(math.log(w) - 0.5 * (D * _LOG_2PI + 2.0 * np.log(np.diag(L)).sum()) - 0.5 * (z * z).sum(axis=0))
        terms = np.stack(terms)
        mx = terms.max(axis=0)
        return mx + np.log(np.exp(terms - mx[None, :]).sum(axis=0))


@dataclass
class MixtureFit:
    """What `mixture_numpy` delivers: the record of nbp_run_mixture (eight entries each, by rank) and what the tests ask of a run"""
    weight: np.ndarray      # 8
    mean: np.ndarray        # 8 x 3
    cov: np.ndarray         # 8 x 3 x 3
    count: np.ndarray       # 8
    labels: np.ndarray      # c
    objective: float
    n_comp: int
    iters: int
    converged: int
    n_dropped: int
    history: list           # J after every iteration
    n_live_min: float       # the least n_k a live component had at an M-step (inf: none)
    n_drop_max: float       # the greatest n_k a component was dropped at (-inf: none)
    resp: np.ndarray        # c x 8, the final responsibilities by STARTING index
    rank: np.ndarray        # 8, starting index -> rank (-1: not live)


def check_options(tol, max_iter, max_components=1):
    """the refusals of nbp_run_mixture and of the Python layer, as ValueErrors"""
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError("mixture: tol must be finite and not negative")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("mixture: maxIter must be an integer >= 1")
    if int(max_components) != max_components or not 1 <= max_components <= MIX_MAX:
        raise ValueError(f"mixture: maxComponents must be an integer in 1 .. {MIX_MAX}")


def _exp_nonpos(a):
    """exp(a), exactly 0 below -700 (mix_exp of csrc/nbp_mixture.h)"""
    with np.errstate(under="ignore"):
        return np.where(a < -700, a.dtype.type(0), np.exp(np.maximum(a, a.dtype.type(-745))))


def _block_sums(V):
    """the columns of V (c x m) added as block_sum of csrc/nbp_device.h adds its lanes (likelihood.block_sum_numpy, column by column
    at once): a butterfly inside every group of 64 rows, then the groups in order"""
    n = -(-V.shape[0] // 64) * 64
    w = np.zeros((n, V.shape[1]), dtype=V.dtype)
    w[:V.shape[0]] = V
    w = w.reshape(-1, 64, V.shape[1])
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, idx ^ o]
    t = w[0, 0]
    for g in range(1, w.shape[0]):
        t = t + w[g, 0]
    return t


def mixture_numpy(manifold, X, bw, labels, init_mean, tol=abi.MIX_TOL, max_iter=abi.MIX_MAX_ITER, dtype=np.float64, at=None):
    """the definition on the host, operation by operation as csrc/nbp_mixture.h writes it, in the arithmetic `dtype` (np.longdouble:
    the measure of a case's conditioning).  X: tangent coordinates (c x D); labels: c starting labels; init_mean: 8 x 3 (or K x D)
    starting means -> MixtureFit.  at: iteration counts -> {t: the MixtureFit of the run with max_iter = t} of ONE pass (a run
    is the prefix of a longer one; a stop by `tol` ends the pass, and later counts hold the stopped result)"""
    check_options(tol, max_iter)
    T = dtype
    D = abi.MANIFOLD_DIM[manifold]
    X = np.asarray(X, dtype=np.float64).reshape(-1, D).astype(T)
    c = X.shape[0]
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)[:c]
    if lab.size != c or np.any(lab < -1) or np.any(lab >= MIX_MAX):
        raise ValueError(f"mixture: one label in -1 .. {MIX_MAX - 1} per point")
    h = np.asarray(bw, dtype=np.float64).reshape(-1)[:D]
    mu0 = np.zeros((MIX_MAX, abi.MAXD))
    im = np.asarray(init_mean, dtype=np.float64)
    mu0[:im.shape[0], :im.shape[1]] = im
    mu = mu0.astype(T)
    circ = _circular(manifold)
    live = [bool(np.any(lab == k)) for k in range(MIX_MAX)]
    valid = len(h) == D and bool(np.all(np.isfinite(h) & (h > 0))) and any(live)
    nan = float("nan")
    if not valid:
        fit = MixtureFit(np.full(MIX_MAX, nan), np.full((MIX_MAX, 3), nan), np.full((MIX_MAX, 3, 3), nan), np.zeros(MIX_MAX, dtype=np.int32),
                         np.full(c, -1, dtype=np.int32), nan, 0, 0, 0, 0, [], math.inf, -math.inf, np.zeros((c, MIX_MAX)),
                         np.full(MIX_MAX, -1, dtype=np.int32))
        return fit if at is None else {t: fit for t in at}
    h = h.astype(T)
    hh = np.zeros(3, dtype=T)
    hh[:D] = h * h
    log_2pi = T(_LOG_2PI) if T is np.float64 else np.log(T(2) * np.arccos(T(-1)))
    half, zero, one = T(0.5), T(0), T(1)
    r = np.zeros((c, MIX_MAX), dtype=T)
    r[np.flatnonzero(lab >= 0), lab[lab >= 0]] = one
    nk = np.zeros(MIX_MAX, dtype=T)
    sig = np.zeros((MIX_MAX, 3, 3), dtype=T)
    pairs = [(d, e) for e in range(D) for d in range(e + 1)]  # 00 01 11 02 12 22: (r delta_d) delta_e

    def delta(k, d):
        dl = X[:, d] - mu[k, d]
        return _wrap(dl, T) if circ[d] else dl

    J, hist, it, dropped, conv = T(nan), [], 0, 0, 0
    n_live_min, n_drop_max = math.inf, -math.inf
    tot = zero

    def finish():
        ks = sorted((k for k in range(MIX_MAX) if live[k]), key=lambda k: (-nk[k], k))
        rank = np.full(MIX_MAX, -1, dtype=np.int32)
        rank[ks] = np.arange(len(ks))
        best = np.argmax(np.where(np.asarray(live)[None, :], r, T(-1)), axis=1)  # (the first of equal maxima: the lower index)
        weight, mean, cov = np.zeros(MIX_MAX, dtype=T), np.zeros((MIX_MAX, 3), dtype=T), np.zeros((MIX_MAX, 3, 3), dtype=T)
        count = np.zeros(MIX_MAX, dtype=np.int32)
        for q, k in enumerate(ks):
            weight[q] = nk[k] / tot
            mean[q, :D] = mu[k, :D]
            cov[q, :D, :D] = sig[k, :D, :D]
            count[q] = int((best == k).sum())
        return MixtureFit(weight, mean, cov, count, rank[best].astype(np.int32), J, len(ks), it, conv, dropped, list(hist), n_live_min,
                          n_drop_max, r.copy(), rank)

    out = {}
    last = max(at) if at is not None else max_iter
    while it < last and not conv:
        it += 1
        ks = [k for k in range(MIX_MAX) if live[k]]
        nk[ks] = _block_sums(r[:, ks])
        tot = zero
        for k in ks:
            if nk[k] < half:
                live[k] = False
                dropped += 1
                n_drop_max = max(n_drop_max, float(nk[k]))
            else:
                tot = tot + nk[k]
                n_live_min = min(n_live_min, float(nk[k]))
        ks = [k for k in range(MIX_MAX) if live[k]]
        step = _block_sums(np.stack([r[:, k] * delta(k, d) for k in ks for d in range(D)], axis=1)).reshape(len(ks), D)
        for q, k in enumerate(ks):
            for d in range(D):
                v = mu[k, d] + step[q, d] / nk[k]
                mu[k, d] = _wrap(v, T) if circ[d] else v
        cols = []
        for k in ks:
            dl = [delta(k, d) for d in range(D)]
            rd = [r[:, k] * dl[d] for d in range(D)]
            cols += [rd[d] * dl[e] for d, e in pairs]
        sc = _block_sums(np.stack(cols, axis=1)).reshape(len(ks), len(pairs))
        for q, k in enumerate(ks):
            S = np.eye(3, dtype=T)
            for j, (d, e) in enumerate(pairs):
                S[d, e] = S[e, d] = sc[q, j] / nk[k] + (hh[d] if d == e else zero)
            sig[k] = S
        l = np.full((c, MIX_MAX), -np.inf, dtype=T)
        for k in ks:
            g = sig[k]
            l00 = np.sqrt(g[0, 0])
            i0 = one / l00
            l10 = g[0, 1] * i0
            l11 = np.sqrt(g[1, 1] - l10 * l10)
            i1 = one / l11
            l20 = g[0, 2] * i0
            l21 = (g[1, 2] - l20 * l10) * i1
            l22 = np.sqrt((g[2, 2] - l20 * l20) - l21 * l21)
            i2 = one / l22
            m10 = -(l10 * i0) * i1
            m21 = -(l21 * i1) * i2
            m20 = -(l20 * i0 + l21 * m10) * i2
            p00, p11, p22 = (i0 * i0 + m10 * m10) + m20 * m20, i1 * i1 + m21 * m21, i2 * i2
            tr = (hh[0] * p00 + hh[1] * p11) + hh[2] * p22
            logdet = T(2) * ((np.log(l00) + np.log(l11)) + np.log(l22))
            cst = np.log(nk[k] / tot) - half * ((T(D) * log_2pi + logdet) + tr)
            d0 = delta(k, 0)
            d1 = delta(k, 1) if D > 1 else np.zeros(c, dtype=T)
            d2 = delta(k, 2) if D > 2 else np.zeros(c, dtype=T)
            z0 = d0 * i0
            z1 = (d1 - l10 * z0) * i1
            z2 = ((d2 - l20 * z0) - l21 * z1) * i2
            l[:, k] = cst - half * ((z0 * z0 + z1 * z1) + z2 * z2)
        mx = l[:, ks].max(axis=1)
        acc = np.zeros(c, dtype=T)
        for k in ks:
            acc = acc + _exp_nonpos(l[:, k] - mx)
        lse = mx + np.log(acc)
        r = np.zeros((c, MIX_MAX), dtype=T)
        for k in ks:
            r[:, k] = _exp_nonpos(l[:, k] - lse)
        Jprev, J = J, _block_sums(lse[:, None])[0] / T(c)
        hist.append(float(J))
        conv = int(tol > 0 and it >= 2 and J - Jprev <= T(tol))
        if at is not None and it in at:
            out[it] = finish()
    if at is None:
        return finish()
    end = finish()
    return {t: out.get(t, end) for t in at}


def starting_from_modes(bm, max_components):
    """the start of a fit from the modes of the belief -> (labels[c], init_mean[8, 3]): the `max_components` most populous modes
    (their rank is the label, their location the starting mean); the particles of the remaining modes get -1"""
    K = min(int(bm.n_modes), int(max_components), len(bm.modes))
    lab = np.asarray(bm.labels, dtype=np.int32).copy()
    lab[lab >= K] = -1
    mu = np.zeros((MIX_MAX, abi.MAXD))
    if K:
        mu[:K, :bm.modes.shape[1]] = bm.modes[:K]
    return lab, mu


def mixture_from_record(manifold, rec, labels, c, modes=None):
    """one belief's row of `HipBackend.run_mixture` (or a MixtureFit) -> BeliefMixture; c: the points the belief holds"""
    D = abi.MANIFOLD_DIM[manifold]
    get = (lambda f: rec[f]) if isinstance(rec, np.void) else (lambda f: getattr(rec, f))
    K = int(get("n_comp"))
    f64 = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
    return BeliefMixture(manifold, f64(get("weight")[:K]), f64(get("mean")[:K, :D]), f64(get("cov")[:K, :D, :D]),
                         np.array(get("count")[:K], dtype=np.int32), np.array(labels[:c], dtype=np.int32), float(get("objective")),
                         int(get("iters")), bool(get("converged")), int(get("n_dropped")), modes)


def _options(maxComponents, bwScale, tol, maxIter):
    check_options(tol, maxIter, maxComponents)
    mode_kw = _mode_options(bwScale, abi.MODES_TOL, abi.MODES_MAX_ITER, abi.MODES_MERGE)
    return int(maxComponents), mode_kw, dict(tol=float(tol), max_iter=int(maxIter))


def mixture_host(manifold, pts, bw, maxComponents, mode_kw, kw):
    """modes_numpy, then mixture_numpy: the whole query on the host"""
    bm = modes_numpy(manifold, pts, bw, **mode_kw)
    lab, mu = starting_from_modes(bm, maxComponents)
    fit = mixture_numpy(manifold, ppe_coords(manifold, pts), bw, lab, mu, **kw)
    return mixture_from_record(manifold, fit, fit.labels, len(fit.labels), bm)


def belief_mixture(manifold, pts, bw, maxComponents=abi.MIX_MAX, bwScale=abi.MODES_BW_SCALE, tol=abi.MIX_TOL, maxIter=abi.MIX_MAX_ITER,
                   backend=None):
    """the mixture summary of a belief held on the host.  `backend`: a HIP backend (class, factory or instance: nbp_kde_modes, then
    nbp_kde_mixture, through slot 0); anything without that entry point, or None: numpy."""
    K, mode_kw, kw = _options(maxComponents, bwScale, tol, maxIter)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[manifold])
    with _backend(backend, len(pts), 1, "kde_mixture") as be:
        if be is None:
            return mixture_host(manifold, pts, bw, K, mode_kw, kw)
        bm = modes_from_records(manifold, *be.kde_modes(manifold, pts, bw, **mode_kw), len(pts))
        lab, mu = starting_from_modes(bm, K)
        rec, out = be.kde_mixture(manifold, pts, bw, lab, mu, **kw)
        return mixture_from_record(manifold, rec, out, len(pts), bm)


def fitBeliefMixture(fg, label, maxComponents=abi.MIX_MAX, bwScale=abi.MODES_BW_SCALE, tol=abi.MIX_TOL, maxIter=abi.MIX_MAX_ITER,
                     backend=None):
    """the variable's current belief as a Gaussian mixture of at most `maxComponents` (1 .. 8) components -> BeliefMixture.  The fit
    starts from the belief's modes at the bandwidth bwScale * bw (modes.py); tol, maxIter: the stopping rule of the EM.  `backend` as
    in calcPPE."""
    v = fg.getVariable(label)
    return belief_mixture(v.varType.manifold, v.val, v.bw, maxComponents, bwScale, tol, maxIter, backend)


def resident_mixtures(be, slots, manifolds, counts, K, mode_kw, kw):
    """the beliefs in `slots` of a HIP backend -> [BeliefMixture]: ONE run_modes, then ONE run_mixture; counts: the points each holds"""
    res = be.run_modes(slots, manifolds, **mode_kw)
    bms = [modes_from_records(m, *(r[i] for r in res), c) for i, (m, c) in enumerate(zip(manifolds, counts))]
    lab = np.full((len(slots), be.N), -1, dtype=np.int32)
    mu = np.zeros((len(slots), MIX_MAX, abi.MAXD))
    for i, bm in enumerate(bms):
        li, mu[i] = starting_from_modes(bm, K)
        lab[i, :len(li)] = li
    recs, out = be.run_mixture(slots, manifolds, lab, mu, **kw)
    return [mixture_from_record(m, recs[i], out[i], c, bms[i]) for i, (m, c) in enumerate(zip(manifolds, counts))]


def fitBeliefMixtureAll(fg, labels=None, maxComponents=abi.MIX_MAX, bwScale=abi.MODES_BW_SCALE, tol=abi.MIX_TOL, maxIter=abi.MIX_MAX_ITER,
                        backend=None):
    """-> {label: BeliefMixture} (labels: default every variable, in natural order).  On a HIP backend the beliefs are written to
    slots 0 .. L-1, ONE run_modes finds the starts and ONE run_mixture fits all of them; otherwise numpy."""
    K, mode_kw, kw = _options(maxComponents, bwScale, tol, maxIter)
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    vs = [fg.getVariable(v) for v in labels]
    if not vs:
        return {}
    mans = [v.varType.manifold for v in vs]
    with _staged(fg, labels, backend, "run_mixture") as (be, _):
        if be is None:
            return {l: mixture_host(m, v.val, v.bw, K, mode_kw, kw) for l, m, v in zip(labels, mans, vs)}
        return dict(zip(labels, resident_mixtures(be, list(range(len(vs))), mans, [len(v.val) for v in vs], K, mode_kw, kw)))
