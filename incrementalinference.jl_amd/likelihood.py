"""Factor likelihoods: how well the current beliefs of a factor's variables explain its measurement model.

Three questions a user asks right after `solveTree` are this one quantity: which association of a multihypo factor won (the
posterior weight of each hypothesis), which Mixture component explains the data (the responsibilities), and which factor
disagrees with the solution (rank the factors by `loglik`: a wrong loop closure comes last).  The reference has no such function --
its nearest tools are `approxDeconv` + `mmd`, one factor at a time and refused for multihypo factors -- so this query is DEFINED
here and unpinned ("Factor likelihoods", and 8).  For the closed set of factors the predicted measurement has a closed
form, so no per-particle search is needed.

The definition, for one ITEM (measurement model, belief A, belief B; B absent for a prior), a_i and b_j in tangent coordinates
(SE(2): x, y, theta), n_a and n_b the counts (n_b = 1 for a prior); bandwidths are never read:

  zhat(a_i, b_j)   LinearRelative b - a | CircularCircular wrap(b - a) | SE(2) (c dx + s dy, -s dx + c dy, wrap(b_th - a_th)) with
                   (s, c) = sincos(a_th) | EuclidDistance sqrt(sum_d (b_d - a_d)^2) | Prior a_i; a partial factor keeps its
                   coordinates, in ascending order
  log p_c(z)       Gaussian: delta = z - mean (wrapped on circular coordinates), L u = delta by forward substitution,
                   -1/2 sum_k u_k^2 - (zd log(2 pi) / 2 + sum_k log L_kk); Uniform(a, a + w): -log w inside, -inf outside;
                   Rayleigh(sigma): (log z - 2 log sigma) - z^2 / (2 sigma^2) for z > 0, else -inf
  e_ijc            log(w_c / sum w) + log p_c(zhat_ij)
  M, S_c           M = max_ijc e_ijc; S_c = sum_i sum_j exp(e_ijc - M), terms below exp(-700) dropped, j in order for every i, the
                   rows added as libnbp's block sum adds its lanes (butterfly inside groups of 64, the groups in order)
  loglik           (M + log sum_c S_c) - log(n_a n_b);  comp_loglik[c] = (M + log S_c) - log(n_a n_b)

finite where every density underflows, -inf where nothing lies in the support, NaN for a belief without points.  Posterior weights
are host arithmetic on these numbers (`hypothesis_weights`, `component_weights`): pi_k proportional to p_k exp(l_k) over the
fractional variables of a multihypo factor -- the null hypothesis has no likelihood and stays out --, responsibilities
exp(comp_loglik[c] - loglik).

On a HIP backend every item of every factor is ONE kernel launch (`HipBackend.run_factor_likelihood`, csrc/nbp_likelihood.h);
`factor_likelihood_numpy` restates the definition on the host in the same pass structure and j order and serves wherever no such
backend is given -- never as a fallback on a device failure."""
import math
from dataclasses import dataclass

import numpy as np

from . import abi
from .beliefquery import _staged
from .ppe import _natural, ppe_coords

_HALF_LOG_2PI = 0.91893853320467274178  # NBP_LIK_HALF_LOG_2PI of csrc/nbp_likelihood.h
_UNARY = (abi.F_PRIOR,)
_KINDS = (abi.F_PRIOR, abi.F_LINREL, abi.F_CIRCULAR, abi.F_SE2, abi.F_EUCLIDDIST)


@dataclass
class FactorLikelihood:
    """The likelihood of one factor.  A plain factor has no hypotheses: `hypotheses` is empty, the `hypo_*` arrays too, and
    `comp_loglik` / `comp_weights` hold one entry per Mixture component (one entry for a factor that is no Mixture).  A multihypo
    factor has one hypothesis per fractional variable: `loglik` = log sum_k p_k exp(l_k), and `comp_*` are K x ncomp."""
    loglik: float
    hypotheses: list          # the labels of the fractional variables, in variable order
    hypo_loglik: np.ndarray   # l_k: the loglik of the item with variable k in its role
    hypo_prior: np.ndarray    # p_k: the normalised fractional entries of `multihypo`
    hypo_weights: np.ndarray  # pi_k
    comp_loglik: np.ndarray
    comp_weights: np.ndarray  # the responsibilities of the Mixture components


class FactorLikelihoods(dict):
    """{factor label: FactorLikelihood} in natural order; `.skipped`: the labels left out as unsupported"""

    def __init__(self, *a, skipped=(), **kw):
        super().__init__(*a, **kw)
        self.skipped = list(skipped)


# ------------------------------------------------------------------------------------------------
# descriptors
# ------------------------------------------------------------------------------------------------
def likelihood_desc(kind, manifold, comps, partial_mask=0, slot_a=0, slot_b=-1):
    """abi.LikelihoodDesc from a measurement model: comps = [(weight, mean, sqrtcov[, family]), ...] as `fnc.components()` gives
    them; entries of sqrtcov above the diagonal are carried as they are, for the check to refuse"""
    if not 1 <= len(comps) <= abi.MAXC:
        raise ValueError("ncomp outside 1 .. NBP_MAXC")
    d = abi.LikelihoodDesc()
    d.kind, d.manifold, d.slot_a, d.slot_b, d.ncomp, d.partial_mask = int(kind), int(manifold), int(slot_a), int(slot_b), len(comps), int(partial_mask)
    for c, comp in enumerate(comps):
        w, mu, L = comp[0], np.atleast_1d(np.asarray(comp[1], dtype=float)), np.atleast_2d(np.asarray(comp[2], dtype=float))
        row = [0.0] * abi.COMP_STRIDE
        row[0] = float(w)
        for i in range(min(3, len(mu))):
            row[1 + i] = float(mu[i])
        for i in range(min(3, L.shape[0])):
            for j in range(min(3, L.shape[1])):
                row[4 + 3 * i + j] = float(L[i, j])
        if len(comp) > 3 and comp[3] != abi.DIST_GAUSSIAN:
            if len(mu) != 1:
                raise ValueError("Uniform / Rayleigh / AliasingScalarSampler measurements are scalar")
            row[12] = float(comp[3])
        d.comp[c][:] = row
    return d


def _mask_zd(d):
    D = abi.MANIFOLD_DIM[d.manifold]
    full = 1 if d.kind in (abi.F_CIRCULAR, abi.F_EUCLIDDIST) else (1 << D) - 1
    mask = d.partial_mask if d.partial_mask else full
    return mask, bin(mask).count("1")


def check_desc(d):
    """the refusals of nbp_run_factor_likelihood (the slots apart), as ValueErrors"""
    def posfin(v):
        return v > 0 and math.isfinite(v)
    if d.kind in (abi.F_MSGPRIOR, abi.F_PASSTHROUGH):
        raise ValueError("message priors and pass-through priors have no density in closed form")
    if d.kind not in _KINDS:
        raise ValueError("unknown factor kind")
    if d.manifold not in abi.MANIFOLD_DIM:
        raise ValueError("unknown manifold")
    if d.kind == abi.F_CIRCULAR and d.manifold != abi.CIRCULAR:
        raise ValueError("CircularCircular needs Circular variables")
    if d.kind == abi.F_SE2 and d.manifold != abi.SE2:
        raise ValueError("SE2 factor needs SE2 variables")
    if d.kind in (abi.F_LINREL, abi.F_EUCLIDDIST) and d.manifold > abi.EUCLID3:
        raise ValueError("LinearRelative and EuclidDistance need Euclid variables")
    if not 1 <= d.ncomp <= abi.MAXC:
        raise ValueError("ncomp outside 1 .. NBP_MAXC")
    D = abi.MANIFOLD_DIM[d.manifold]
    if d.partial_mask:
        if d.partial_mask < 0 or d.partial_mask >= (1 << D):
            raise ValueError("partial_mask outside the manifold's coordinates")
        if d.kind == abi.F_LINREL:
            if bin(d.partial_mask).count("1") > 2:
                raise ValueError("partial LinearRelative: one or two partial coordinates")
        elif d.kind not in (abi.F_PRIOR, abi.F_SE2):
            raise ValueError("partial_mask is supported for Prior, LinearRelative and SE(2) ManifoldFactor factors")
    _, zd = _mask_zd(d)
    wsum = 0.0
    for c in range(d.ncomp):
        q = d.comp[c]
        if not (q[0] >= 0 and math.isfinite(q[0])):
            raise ValueError("a component weight is negative or not finite")
        wsum += q[0]
        fam = q[12] if zd == 1 else 0.0
        if fam == abi.DIST_TABLE:
            raise ValueError("an alias table has no density")
        if fam not in (abi.DIST_GAUSSIAN, abi.DIST_UNIFORM, abi.DIST_RAYLEIGH):
            raise ValueError("unknown measurement family")
        if fam == abi.DIST_UNIFORM:
            if not posfin(q[4]):
                raise ValueError("the width of a Uniform is not positive and finite")
        elif fam == abi.DIST_RAYLEIGH:
            if not posfin(q[4]):
                raise ValueError("the sigma of a Rayleigh is not positive and finite")
        else:
            for i in range(zd):
                if not posfin(q[4 + 3 * i + i]):
                    raise ValueError("a diagonal entry of L is not positive and finite")
                for j in range(i + 1, zd):
                    if q[4 + 3 * i + j] != 0.0:
                        raise ValueError("L has a non-zero above the diagonal")
    if not (wsum > 0 and math.isfinite(wsum)):
        raise ValueError("the component weights have no positive sum")


# ------------------------------------------------------------------------------------------------
# the definition on the host
# ------------------------------------------------------------------------------------------------
def _wrap(x, T):
    """to [-pi, pi), the identity on that interval (nbpm_wrap_pi of include/nbp_math.h), in the arithmetic T"""
    pi = T(np.pi)
    return np.where((x >= -pi) & (x < pi), x, (x + pi) % (T(2) * pi) - pi)


def _coords(manifold, pts, T):
    """host points (n x P) -> tangent coordinates (n x D); SE(2) points may also come as n x 3 tangent coordinates"""
    D, P = abi.MANIFOLD_DIM[manifold], abi.MANIFOLD_P[manifold]
    pts = np.asarray(pts, dtype=np.float64)
    if manifold == abi.SE2 and pts.ndim == 2 and pts.shape[1] == D:
        return np.ascontiguousarray(pts).astype(T)
    return np.ascontiguousarray(ppe_coords(manifold, pts.reshape(-1, P))).astype(T)


def block_sum_numpy(v):
    """the rows added as block_sum of csrc/nbp_device.h adds its lanes: a butterfly (xor 32, 16, .. 1) inside every group of 64, then
    the groups in order.  Lanes beyond the count add zeros, so the value does not depend on the workgroup's size."""
    v = np.asarray(v)
    n = -(-v.shape[0] // 64) * 64
    w = np.zeros(n, dtype=v.dtype)
    w[:v.shape[0]] = v
    w = w.reshape(-1, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, idx ^ o]
    t = w[0, 0]
    for g in range(1, w.shape[0]):
        t = t + w[g, 0]
    return t


def predicted_measurement(desc, A, B=None, dtype=np.float64):
    """zhat(a_i, b_j) of the definition -> [zd arrays of shape (n_a, n_b)] (a prior: (n_a, 1)) and the circular flag of each"""
    T = dtype
    kind, M = desc.kind, desc.manifold
    D = abi.MANIFOLD_DIM[M]
    a = _coords(M, A, T)
    if kind in _UNARY:
        f = [a[:, d, None] for d in range(D)]
        circ = [(M == abi.CIRCULAR and d == 0) or (M == abi.SE2 and d == 2) for d in range(D)]
    else:
        b = _coords(M, B, T)
        df = [b[None, :, d] - a[:, None, d] for d in range(D)]
        if kind == abi.F_LINREL:
            f, circ = df, [False] * D
        elif kind == abi.F_CIRCULAR:
            f, circ = [_wrap(df[0], T)], [True]
        elif kind == abi.F_SE2:
            s, c = np.sin(a[:, 2])[:, None], np.cos(a[:, 2])[:, None]
            f = [c * df[0] + s * df[1], -s * df[0] + c * df[1], _wrap(df[2], T)]
            circ = [False, False, True]
        else:
            q = df[0] * df[0]
            for d in range(1, D):
                q = q + df[d] * df[d]
            f, circ = [np.sqrt(q)], [False]
    mask, _ = _mask_zd(desc)
    sel = [k for k in range(3) if mask >> k & 1]
    return [f[k] for k in sel], [circ[k] for k in sel]


def pair_terms(desc, A, B=None, dtype=np.float64):
    """e_ijc of the definition -> [ncomp arrays of shape (n_a, n_b)] (a prior: (n_a, 1)), in the arithmetic `dtype`"""
    T = dtype
    z, circ = predicted_measurement(desc, A, B, T)
    zd, ncomp = len(z), desc.ncomp
    wsum = T(0)
    for c in range(ncomp):
        wsum = wsum + T(desc.comp[c][0])
    e = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(ncomp):
            q = [T(v) for v in desc.comp[c]]
            logw = np.log(q[0] / wsum) if q[0] > 0 else T(-np.inf)
            fam = int(q[12]) if zd == 1 else abi.DIST_GAUSSIAN
            if fam == abi.DIST_UNIFORM:
                lp = np.where((z[0] >= q[1]) & (z[0] <= q[1] + q[4]), -np.log(q[4]), T(-np.inf))
            elif fam == abi.DIST_RAYLEIGH:
                inside = z[0] > 0
                v = (np.log(np.where(inside, z[0], T(1))) - T(2) * np.log(q[4])) - (z[0] * z[0]) / (T(2) * (q[4] * q[4]))
                lp = np.where(inside, v, T(-np.inf))
            else:
                u, acc, s = [], None, T(0)
                for k in range(zd):
                    dl = z[k] - q[1 + k]
                    if circ[k]:
                        dl = _wrap(dl, T)
                    for j in range(k):
                        dl = dl - q[4 + 3 * k + j] * u[j]
                    u.append(dl / q[4 + 3 * k + k])
                    acc = u[k] * u[k] if acc is None else acc + u[k] * u[k]
                    s = np.log(q[4 + 3 * k + k]) if k == 0 else s + np.log(q[4 + 3 * k + k])
                lp = T(-0.5) * acc - (T(zd) * T(_HALF_LOG_2PI) + s)
            e.append((logw + lp).astype(T))
    return e


def shifted_exp(dl, T):
    """exp(e - M) as pass 2 takes it: a term below exp(-700) counts as zero"""
    return np.where(dl >= -700, np.exp(np.maximum(dl, T(-745))), T(0))


def factor_likelihood_numpy(desc, A, B=None, dtype=np.float64):
    """the definition on the host, in the arithmetic `dtype` (np.longdouble: the measure of a case's conditioning).  desc: an
    abi.LikelihoodDesc (or anything with its fields; the slots are not read); A, B: the host points of the two roles (n x P; SE(2)
    also n x 3 tangent coordinates), B None for a prior -> (loglik, comp_loglik[4]), entries beyond ncomp NaN"""
    check_desc(desc)
    T = dtype
    unary = desc.kind in _UNARY
    if not unary and B is None:
        raise ValueError("a relative factor has two roles")
    M = desc.manifold
    na = _coords(M, A, T).shape[0]
    nb = 1 if unary else _coords(M, B, T).shape[0]
    cl = np.full(abi.MAXC, np.nan, dtype=T)
    if na == 0 or nb == 0:
        return T(np.nan), cl
    e, ncomp = pair_terms(desc, A, B, T), desc.ncomp
    with np.errstate(divide="ignore", invalid="ignore"):
        Mx = max(x.max() for x in e)
        if not Mx > -np.inf:
            cl[:ncomp] = -np.inf
            return T(-np.inf), cl
        ln = np.log(T(na) * T(nb))
        tot = T(0)
        for c in range(ncomp):
            w = shifted_exp(e[c] - Mx, T)
            S = block_sum_numpy(np.cumsum(w, axis=1)[:, -1])  # (a cumulative sum along j is the running sum in j order)
            tot = tot + S
            cl[c] = (Mx + np.log(S)) - ln if S > 0 else -np.inf
        return ((Mx + np.log(tot)) - ln if tot > 0 else T(-np.inf)), cl


# ------------------------------------------------------------------------------------------------
# posterior weights
# ------------------------------------------------------------------------------------------------
def _logsumexp(logs, p=None):
    logs = np.asarray(logs, dtype=np.float64)
    m = logs.max()
    if not m > -np.inf:
        return float(m)  # all -inf (or NaN)
    w = np.exp(logs - m) if p is None else np.asarray(p, dtype=np.float64) * np.exp(logs - m)
    return float(m + math.log(w.sum()))


def hypothesis_weights(prior, logliks):
    """pi_k proportional to p_k exp(l_k), formed by max-shift; all -inf: NaN"""
    prior, logliks = np.asarray(prior, dtype=np.float64), np.asarray(logliks, dtype=np.float64)
    if logliks.size == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore"):
        w = prior * np.exp(logliks - logliks.max())
        return w / w.sum()


def component_weights(comp_loglik):
    """the responsibilities exp(comp_loglik[c] - loglik) of the Mixture components, formed by max-shift; all -inf: NaN"""
    return hypothesis_weights(np.ones(len(comp_loglik)), comp_loglik)


# ------------------------------------------------------------------------------------------------
# a factor of a graph as items
# ------------------------------------------------------------------------------------------------
@dataclass
class _Plan:
    label: str
    descs: list       # one abi.LikelihoodDesc per item, the slots not yet set
    roles: list       # per item: (label a, label b or None)
    hypotheses: list  # the labels of the fractional variables ([] for a plain factor)
    prior: np.ndarray


def factor_items(fg, label):
    """the items of one factor: the measurement model from `fnc.components()`, the mask from its partial, the roles a / b filled in
    getVariableOrder order; a multihypo factor gives one item per fractional variable k, its roles filled by the certain variable
    and variable k in variable order.  ValueError naming the factor for anything nbp_run_factor_likelihood refuses, and for
    selected variables that do not match the kind's arity."""
    fct = fg.getFactor(label)
    fnc = fct.fnc
    try:
        kind = fnc.kind
        if getattr(fnc, "meas_slot", None) is not None:
            raise ValueError("a measurement held as a KDE has no density in closed form")
        if kind in (abi.F_MSGPRIOR, abi.F_PASSTHROUGH):
            raise ValueError("message priors and pass-through priors have no density in closed form")
        if kind not in _KINDS:
            raise ValueError("unknown factor kind")
        if getattr(fnc, "table", None) is not None:
            raise ValueError("an alias table has no density")
        arity = 1 if kind in _UNARY else 2
        names = list(fct.variables)
        if fct.multihypo is not None:
            mh = np.asarray(fct.multihypo, dtype=np.float64)
            certain = [i for i in range(len(names)) if mh[i] == 0.0]
            frac = [i for i in range(len(names)) if mh[i] > 0.0]
            if len(certain) != arity - 1 or not frac:
                raise ValueError(f"the certain variables of the multihypo factor do not fill the {arity - 1} other role(s) of its kind")
            picks = [sorted(certain + [k]) for k in frac]
            hypotheses, prior = [names[k] for k in frac], mh[frac] / mh[frac].sum()
        else:
            if len(names) != arity:
                raise ValueError(f"{len(names)} variable(s) for a factor of arity {arity}")
            picks, hypotheses, prior = [list(range(arity))], [], np.zeros(0)
        descs, roles = [], []
        for pick in picks:
            mans = {fg.getVariable(names[i]).varType.manifold for i in pick}
            if len(mans) != 1:
                raise ValueError("the variables of an item lie on different manifolds")
            d = likelihood_desc(kind, mans.pop(), fnc.components(), getattr(fnc, "partial_mask", 0))
            check_desc(d)
            descs.append(d)
            roles.append((names[pick[0]], names[pick[1]] if arity == 2 else None))
    except ValueError as err:
        raise ValueError(f"factorLikelihood: factor {label}: {err}") from None
    return _Plan(label, descs, roles, hypotheses, prior)


def assemble(plan, loglik, comp_loglik):
    """the items' numbers (loglik[K], comp_loglik[K, 4]) of one factor -> FactorLikelihood"""
    ll = np.array(loglik, dtype=np.float64).reshape(-1)
    ncomp = plan.descs[0].ncomp
    cl = np.array(comp_loglik, dtype=np.float64).reshape(len(ll), -1)[:, :ncomp]
    cw = np.stack([component_weights(r) for r in cl])
    if not plan.hypotheses:
        return FactorLikelihood(float(ll[0]), [], np.zeros(0), np.zeros(0), np.zeros(0), cl[0], cw[0])
    return FactorLikelihood(_logsumexp(ll, plan.prior), list(plan.hypotheses), ll, plan.prior.copy(),
                            hypothesis_weights(plan.prior, ll), cl, cw)


def plan_factors(fg, labels=None, skip_unsupported=True):
    """-> ([_Plan], skipped labels) of the factors `labels` (default: every factor), in natural order"""
    labels = sorted(fg.lsf(), key=_natural) if labels is None else list(labels)
    plans, skipped = [], []
    for l in labels:
        try:
            plans.append(factor_items(fg, l))
        except ValueError:
            if not skip_unsupported:
                raise
            skipped.append(l)
    return plans, skipped


def run_plans(be, plans, place):
    """ONE run_factor_likelihood for every item of every plan, the beliefs read in the slots `place` names -> {label: FactorLikelihood}"""
    descs = []
    for p in plans:
        for d, (a, b) in zip(p.descs, p.roles):
            d.slot_a, d.slot_b = place[a], (-1 if b is None else place[b])
            descs.append(d)
    out = {}
    if not descs:
        return out
    ll, cl = be.run_factor_likelihood(descs)
    at = 0
    for p in plans:
        k = len(p.descs)
        out[p.label] = assemble(p, ll[at:at + k], cl[at:at + k])
        at += k
    return out


def factorLikelihoodAll(fg, labels=None, backend=None, skip_unsupported=True):
    """-> FactorLikelihoods {label: FactorLikelihood} of the factors `labels` (default: every factor) in natural order, with the
    unsupported ones (message and pass-through priors, tables, KDE measurements) listed in `.skipped` -- or, with
    skip_unsupported=False, a ValueError naming the first of them.  On a HIP backend the beliefs of the variables are written once
    and ONE run_factor_likelihood serves every item of every factor; otherwise numpy."""
    plans, skipped = plan_factors(fg, labels, skip_unsupported)
    names = []
    for p in plans:
        for a, b in p.roles:
            names += [v for v in (a, b) if v is not None and v not in names]
    with _staged(fg, names, backend, "run_factor_likelihood") as (be, place):
        if be is None:
            res = {}
            for p in plans:
                got = [factor_likelihood_numpy(d, fg.getVariable(a).val, None if b is None else fg.getVariable(b).val)
                       for d, (a, b) in zip(p.descs, p.roles)]
                res[p.label] = assemble(p, [g[0] for g in got], [g[1] for g in got])
        else:
            res = run_plans(be, plans, place)
        return FactorLikelihoods(((p.label, res[p.label]) for p in plans), skipped=skipped)


def factorLikelihood(fg, fct, backend=None):
    """the likelihood of the factor `fct` under the current beliefs of its variables -> FactorLikelihood.  ValueError naming the
    factor when it is one of the unsupported.  `backend` as in calcPPE."""
    return factorLikelihoodAll(fg, [fct], backend, skip_unsupported=False)[fct]
