"""Joint hypotheses: which mode of one variable belongs with which mode of another, and how probable a whole combination is.

`getBeliefModes` reports that x7 has two modes and that l1 has two modes; belief propagation returns marginals only, so nothing says
which mode of x7 goes with which mode of l1.  This query does (DEFINED here and unpinned: DESIGN.md 3, "Joint hypotheses", and 8).

A particle of a belief carries the rank of its mode (`BeliefModes.labels`), at most `abi.MAXK` = 8 groups per belief; -1 leaves the
particle out.  For one ITEM of a factor (measurement model, belief A, belief B; likelihood.py) and every pair of groups (k, l), with
e_ijc, the wrap rules and the cut-off at -700 exactly as in likelihood.py:

  M_kl      max over i in k, j in l, c of e_ijc
  S_klc     sum_{i in k} sum_{j in l} exp(e_ijc - M_kl): j ascending for every i, the rows added as libnbp's block sum adds its lanes
            with an exact zero in every row outside k, the components then added in ascending c
  T[k, l]   (M_kl + log sum_c S_klc) - log(n_k n_l); -inf where M_kl = -inf; NaN where the cell has no member pair

-- the likelihood of the measurement given "a is in its mode k and b is in its mode l".  A prior has one column.  With one group on
either side T[0, 0] is `factor_likelihood_numpy`'s loglik, bit for bit.

The JOINT SCORE of a choice k = (k_v) of one mode per variable is the sum over the factors of T_f[k_a, k_b] (a prior: T_f[k_a, 0]; a
multihypo factor: logsumexp_h(log p_h + T_fh[k_a, k_bh]), the null hypothesis out as in `factorLikelihood`).  The shares of the modes
do NOT enter: the marginals already contain the factors, and using them would count every measurement twice.  best = argmax score,
logZ = logsumexp_k score(k), weight(k) = exp(score(k) - logZ).  The approximation is that, given the modes, the particles within a
mode of one variable are independent of those within a mode of another.

The pair sums are one kernel launch for every item of every factor on a HIP backend (`HipBackend.run_factor_mode_likelihood`,
csrc/nbp_likelihood.h); `factor_mode_likelihood_numpy` restates the definition in the same summation order.  The discrete problem
over mode indices -- a few states per variable -- is solved exactly on the host by variable elimination
(`joint_modes_from_tables`), on loopy graphs too."""
import math
from dataclasses import dataclass, field

import numpy as np

from . import abi, likelihood
from . import modes as _modes
from .beliefquery import _staged
from .likelihood import _UNARY, _coords, block_sum_numpy, check_desc, pair_terms, shifted_exp
from .ppe import _natural

MAXK = abi.MAXK


# ------------------------------------------------------------------------------------------------
# the definition on the host
# ------------------------------------------------------------------------------------------------
def _labels(lab, n):
    if lab is None:
        return np.zeros(n, dtype=np.int64)
    lab = np.asarray(lab).reshape(-1).astype(np.int64)
    if lab.size != n:
        raise ValueError("one label per point")
    if lab.size and (lab.min() < -1 or lab.max() >= MAXK):
        raise ValueError("a label outside -1 .. NBP_MAXK - 1")
    return lab


def factor_mode_likelihood_numpy(desc, A, labels_a=None, B=None, labels_b=None, dtype=np.float64, terms=None):
    """the definition on the host, in the arithmetic `dtype` (np.longdouble: the measure of a cell's conditioning).  desc, A, B as in
    `factor_likelihood_numpy`; labels_*: one group in -1 .. 7 per point, None: every point in group 0 (labels_b is not read for a
    prior); terms: `pair_terms(desc, A, B, dtype)` where the caller asks about several groupings of the same clouds
    -> (table[8, 8], counts[2, 8])"""
    check_desc(desc)
    T = dtype
    unary = desc.kind in _UNARY
    if not unary and B is None:
        raise ValueError("a relative factor has two roles")
    na = _coords(desc.manifold, A, T).shape[0]
    nb = 1 if unary else _coords(desc.manifold, B, T).shape[0]
    la, lb = _labels(labels_a, na), _labels(None if unary else labels_b, nb)
    table = np.full((MAXK, MAXK), np.nan, dtype=T)
    counts = np.stack([np.bincount(la[la >= 0], minlength=MAXK), np.bincount(lb[lb >= 0], minlength=MAXK)]).astype(np.int32)
    if na == 0 or nb == 0:
        return table, counts
    e = pair_terms(desc, A, None if unary else B, T) if terms is None else terms
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(MAXK):
            rows = np.nonzero(la == k)[0]
            for l in range(MAXK):
                cols = np.nonzero(lb == l)[0]
                if not rows.size or not cols.size:
                    continue
                sub = [x[np.ix_(rows, cols)] for x in e]
                Mx = max(x.max() for x in sub)
                if not Mx > -np.inf:
                    table[k, l] = -np.inf
                    continue
                tot = T(0)
                for x in sub:
                    lanes = np.zeros(na, dtype=T)  # (an exact zero in every lane that is not a member)
                    lanes[rows] = np.cumsum(shifted_exp(x - Mx, T), axis=1)[:, -1]
                    tot = tot + block_sum_numpy(lanes)
                ln = np.log(T(rows.size) * T(cols.size))
                table[k, l] = (Mx + np.log(tot)) - ln if tot > 0 else -np.inf
    return table, counts


# ------------------------------------------------------------------------------------------------
# the tables of the factors of a graph
# ------------------------------------------------------------------------------------------------
@dataclass
class FactorModeLikelihood:
    """The mode-by-mode likelihood of one factor.  `tables[h]` is the K_a x K_b table of item h (a plain factor has one item; a
    prior's table is K_a x 1; a multihypo factor has one item per fractional variable, `hypotheses`, with the normalised priors
    `hypo_prior`); `variables[h]` = (a, b or None) are the variables of its rows and columns."""
    variables: list
    hypotheses: list
    hypo_prior: np.ndarray
    tables: list
    counts: list     # per item: int32[2, 8], the members of every group of the two roles
    coverage: dict   # {variable: the share of its points that carry a kept mode}


class FactorModeLikelihoods(dict):
    """{factor label: FactorModeLikelihood} in natural order; `.skipped`: the labels left out as unsupported"""

    def __init__(self, *a, skipped=(), **kw):
        super().__init__(*a, **kw)
        self.skipped = list(skipped)


def _check_max_modes(maxModes):
    if int(maxModes) != maxModes or not 1 <= maxModes <= MAXK:
        raise ValueError(f"maxModes must be an integer in 1 .. {MAXK}")
    return int(maxModes)


def label_row(bm, maxModes=MAXK):
    """the label row of a belief: the rank of each point's mode; ranks >= maxModes, and the -1 a point without density carries,
    become -1"""
    lab = np.array(bm.labels, dtype=np.int32)
    lab[(lab < 0) | (lab >= maxModes)] = -1
    return lab


def kept_modes(bm, maxModes=MAXK):
    """K_v: the modes of a belief that take part (at least one: a belief without density has one empty group)"""
    return max(1, min(int(bm.n_modes), int(maxModes)))


def _plan_variables(plans):
    names = []
    for p in plans:
        for a, b in p.roles:
            names += [v for v in (a, b) if v is not None and v not in names]
    return names


def assemble_tables(plan, tables, counts, modes, maxModes):
    """the items' tables (each 8 x 8) and counts of one factor -> FactorModeLikelihood"""
    tabs, cov = [], {}
    for (a, b), t in zip(plan.roles, tables):
        ka, kb = kept_modes(modes[a], maxModes), (1 if b is None else kept_modes(modes[b], maxModes))
        tabs.append(np.array(t, dtype=np.float64)[:ka, :kb])
        for v in (a, b):
            if v is not None:
                lab = label_row(modes[v], maxModes)
                cov[v] = float((lab >= 0).sum()) / max(len(lab), 1)
    return FactorModeLikelihood([tuple(r) for r in plan.roles], list(plan.hypotheses), np.array(plan.prior, dtype=np.float64), tabs,
                                [np.array(c, dtype=np.int32) for c in counts], cov)


def run_mode_plans(be, plans, place, modes, maxModes=MAXK):
    """ONE run_factor_mode_likelihood for every item of every plan, the beliefs read in the slots `place` names, the label rows
    those of `modes` -> {label: FactorModeLikelihood}"""
    names = _plan_variables(plans)
    row = {v: i for i, v in enumerate(names)}
    lab = np.full((len(names), be.N), -1, dtype=np.int32)
    for v, i in row.items():
        r = label_row(modes[v], maxModes)[:be.N]
        lab[i, :len(r)] = r
    descs, ra, rb = [], [], []
    for p in plans:
        for d, (a, b) in zip(p.descs, p.roles):
            d.slot_a, d.slot_b = place[a], (-1 if b is None else place[b])
            descs.append(d)
            ra.append(row[a])
            rb.append(-1 if b is None else row[b])
    out = {}
    if not descs:
        return out
    tab, cnt = be.run_factor_mode_likelihood(descs, ra, rb, lab)
    at = 0
    for p in plans:
        k = len(p.descs)
        out[p.label] = assemble_tables(p, tab[at:at + k], cnt[at:at + k], modes, maxModes)
        at += k
    return out


def _numpy_plans(fg, plans, modes, maxModes):
    res = {}
    for p in plans:
        got = [factor_mode_likelihood_numpy(d, fg.getVariable(a).val, label_row(modes[a], maxModes),
                                            None if b is None else fg.getVariable(b).val, None if b is None else label_row(modes[b], maxModes))
               for d, (a, b) in zip(p.descs, p.roles)]
        res[p.label] = assemble_tables(p, [g[0] for g in got], [g[1] for g in got], modes, maxModes)
    return res


def _tables_of(fg, plans, modes, maxModes, backend, mode_kw):
    """the modes of the variables of `plans` (those of `modes` where given, else found here) and the tables of the plans.  On a HIP
    backend the beliefs are written once; one run_modes launch (where modes are to be found) and one table launch follow."""
    names = _plan_variables(plans)
    vs = [fg.getVariable(v) for v in names]
    with _staged(fg, names, backend, "run_factor_mode_likelihood") as (be, place):
        modes = dict(modes) if modes is not None else {}
        missing = [v for v in names if v not in modes]
        if be is None:
            for v in missing:
                var = fg.getVariable(v)
                modes[v] = _modes.modes_numpy(var.varType.manifold, var.val, var.bw, **mode_kw)
            return modes, _numpy_plans(fg, plans, modes, maxModes)
        mans = [v.varType.manifold for v in vs]
        if missing:
            res = be.run_modes([place[v] for v in missing], [mans[place[v]] for v in missing], **mode_kw)
            for i, v in enumerate(missing):
                modes[v] = _modes.modes_from_records(mans[place[v]], *(r[i] for r in res), len(vs[place[v]].val))
        return modes, run_mode_plans(be, plans, place, modes, maxModes)


def factorModeLikelihoodAll(fg, labels=None, modes=None, maxModes=MAXK, backend=None, skip_unsupported=True):
    """-> FactorModeLikelihoods {label: FactorModeLikelihood} of the factors `labels` (default: every factor) in natural order, the
    unsupported ones handled as `factorLikelihoodAll` handles them.  modes: {variable: BeliefModes}; omitted: the modes with the
    default options, found once for all variables.  On a HIP backend the beliefs are written once and every item of every factor
    goes in ONE launch; otherwise numpy."""
    maxModes = _check_max_modes(maxModes)
    plans, skipped = likelihood.plan_factors(fg, labels, skip_unsupported)
    _, res = _tables_of(fg, plans, modes, maxModes, backend, _modes._options(abi.MODES_BW_SCALE, abi.MODES_TOL, abi.MODES_MAX_ITER, abi.MODES_MERGE))
    return FactorModeLikelihoods(((p.label, res[p.label]) for p in plans), skipped=skipped)


def factorModeLikelihood(fg, f, modes=None, maxModes=MAXK, backend=None):
    """the mode-by-mode likelihood of the factor `f` under the current beliefs of its variables -> FactorModeLikelihood.  ValueError
    naming the factor when it is one of the unsupported.  `backend` as in calcPPE."""
    return factorModeLikelihoodAll(fg, [f], modes, maxModes, backend, skip_unsupported=False)[f]


# ------------------------------------------------------------------------------------------------
# the discrete problem over mode indices
# ------------------------------------------------------------------------------------------------
@dataclass
class MultihypoTerm:
    """a multihypo factor as a term of the joint score: logsumexp_h(log prior[h] + table_h[k of variables_h]); items: [(variables,
    table), ...]"""
    prior: np.ndarray
    items: list


@dataclass
class JointSolution:
    """What `joint_modes_from_tables` returns.  `variables`: the unknowns (K_v > 1) in natural order; `best`: {variable: state} for
    every variable of K; combos (C x len(variables)), logscores and weights: every combination, heaviest first, or None where there
    are more than `enumerate_up_to`."""
    variables: list
    best: dict
    best_logscore: float
    logZ: float
    best_weight: float
    combos: np.ndarray = None
    logscores: np.ndarray = None
    weights: np.ndarray = None


def _lse(x, axis=None):
    """logsumexp by max-shift; -inf where everything is -inf"""
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x, axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.log(np.sum(np.exp(x - np.where(np.isfinite(m), m, 0.0)), axis=axis, keepdims=True)) + np.where(np.isfinite(m), m, 0.0)
    s = np.where(m == -np.inf, -np.inf, s)
    return float(s) if axis is None else np.squeeze(s, axis=axis)


def _expand(scope, table, over):
    """a table over `scope` as an array that broadcasts over the variables `over` (a superset, in order)"""
    table = np.asarray(table, dtype=np.float64)
    src = [scope.index(v) for v in over if v in scope]
    t = np.transpose(table, src) if table.ndim else table
    return t.reshape([t.shape[[v for v in over if v in scope].index(v)] if v in scope else 1 for v in over])


def _as_factor(K, variables, table, order_key, cap):
    """(variables, table) -> (scope of unknowns in natural order, array): the variables fixed at one state are indexed away"""
    variables, table = list(variables), np.asarray(table, dtype=np.float64)
    if table.ndim != len(variables) or any(table.shape[i] != K[v] for i, v in enumerate(variables)):
        raise ValueError(f"a table over {variables} has shape {table.shape}, the variables have {[K[v] for v in variables]} states")
    if len(set(variables)) != len(variables):
        raise ValueError(f"a table names a variable twice: {variables}")
    keep = [v for v in variables if K[v] > 1]
    table = table.reshape([K[v] for v in keep])
    scope = sorted(keep, key=order_key)
    return scope, _expand(keep, table, scope)


def _combine(K, parts, order_key, cap):
    """the sum of factors [(scope, array)] as one factor over the union of their scopes; ValueError when it exceeds `cap` entries"""
    scope = sorted({v for s, _ in parts for v in s}, key=order_key)
    size = math.prod(K[v] for v in scope)
    if size > cap:
        raise ValueError(f"jointModes: the table over {scope} would hold {size} entries, more than the cap of {cap}")
    tot = np.zeros([K[v] for v in scope])
    for s, t in parts:
        tot = tot + _expand(s, t, scope)
    return scope, tot


def _term_factor(K, term, order_key, cap):
    if not isinstance(term, MultihypoTerm):
        return _as_factor(K, term[0], term[1], order_key, cap)
    prior = np.asarray(term.prior, dtype=np.float64)
    if len(prior) != len(term.items) or not len(prior):
        raise ValueError("a multihypo term has one prior per item")
    parts = [_as_factor(K, v, t, order_key, cap) for v, t in term.items]
    scope = sorted({v for s, _ in parts for v in s}, key=order_key)
    size = math.prod(K[v] for v in scope)
    if size > cap:
        raise ValueError(f"jointModes: the table over {scope} would hold {size} entries, more than the cap of {cap}")
    shape = [K[v] for v in scope]
    with np.errstate(divide="ignore"):
        stack = np.stack([np.broadcast_to(np.log(p) + _expand(s, t, scope), shape) for p, (s, t) in zip(prior, parts)])
    return scope, _lse(stack, axis=0).reshape(shape)


def _elimination_order(unknowns, factors, order_key):
    """greedy minimum degree, ties by natural label order"""
    adj = {v: set() for v in unknowns}
    for s, _ in factors:
        for v in s:
            adj[v] |= set(s) - {v}
    order = []
    while adj:
        v = min(adj, key=lambda u: (len(adj[u]), order_key(u)))
        nb = adj.pop(v)
        for u in nb:
            adj[u] |= nb - {u}
            adj[u].discard(v)
        order.append(v)
    return order


def _eliminate(K, factors, order, order_key, cap, maximise):
    """variable elimination in (max, +) or (logsumexp, +) -> (value, the argmax records [(v, scope without v, argmax array)])"""
    factors, trace, const = list(factors), [], 0.0
    for v in order:
        mine = [f for f in factors if v in f[0]]
        factors = [f for f in factors if v not in f[0]]
        scope, tot = _combine(K, mine, order_key, cap)
        ax = scope.index(v)
        rest = [u for u in scope if u != v]
        if maximise:
            trace.append((v, rest, np.argmax(tot, axis=ax)))
            red = np.max(tot, axis=ax)
        else:
            red = _lse(tot, axis=ax)
        factors.append((rest, np.asarray(red, dtype=np.float64)))
    for s, t in factors:  # (what is left has an empty scope)
        const = const + float(np.asarray(t).reshape(()))
    return const, trace


def joint_modes_from_tables(K, terms, cap=2**22, enumerate_up_to=4096):
    """The host inference on plain tables.  K: {variable: number of states}; terms: (variables, table) with table of shape
    (K_v for v in variables) -- a prior's column already taken --, or MultihypoTerm.  score(k) = the sum of the terms at k; a
    variable with one state is fixed at 0.  Eliminates the unknowns in (max, +) for `best` and in (logsumexp, +) for `logZ`, in
    greedy minimum-degree order (ties: natural label order); a multihypo term is formed first as a table over the variables it
    touches.  ValueError naming the variables of any intermediate table that would exceed `cap` entries.  With at most
    `enumerate_up_to` combinations, every one of them with its score and weight, heaviest first (equal scores: in the order of the
    combinations).  Every score -inf: best_logscore = -inf and NaN weights.  -> JointSolution"""
    K = {v: int(k) for v, k in K.items()}
    if any(k < 1 for k in K.values()):
        raise ValueError("every variable has at least one state")
    key = _natural
    unknowns = sorted((v for v in K if K[v] > 1), key=key)
    factors = [_term_factor(K, t, key, cap) for t in terms]
    order = _elimination_order(unknowns, factors, key)
    best_score, trace = _eliminate(K, factors, order, key, cap, True)
    logZ, _ = _eliminate(K, factors, order, key, cap, False)
    best = {v: 0 for v in K}
    for v, rest, arg in reversed(trace):
        best[v] = int(arg[tuple(best[u] for u in rest)])
    best = {v: best[v] for v in sorted(K, key=key)}
    with np.errstate(invalid="ignore"):
        sol = JointSolution(unknowns, best, float(best_score), float(logZ), float(np.exp(best_score - logZ)) if logZ > -np.inf else float("nan"))
    n = math.prod(K[v] for v in unknowns)
    if n <= enumerate_up_to:
        shape = [K[v] for v in unknowns]
        score = np.zeros(shape)
        for s, t in factors:
            score = score + _expand(s, t, unknowns)
        flat = score.reshape(-1)
        idx = np.argsort(-flat, kind="stable")
        sol.combos = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64) if unknowns else np.zeros((1, 0), dtype=np.int64)
        sol.logscores = flat[idx]
        with np.errstate(invalid="ignore"):
            sol.weights = np.exp(sol.logscores - logZ) if logZ > -np.inf else np.full(len(idx), np.nan)
    return sol


# ------------------------------------------------------------------------------------------------
# the joint hypothesis of a graph
# ------------------------------------------------------------------------------------------------
@dataclass
class JointModes:
    """The joint hypothesis of a graph.  `variables`: the multimodal variables in natural order; `modes`: the BeliefModes of every
    variable used; `best`: {variable: mode rank} for all of them, `best_points` the location of that mode; combos / logscores /
    weights: every combination of the multimodal variables' modes, heaviest first (None above 4096 combinations); `tables`:
    {factor: FactorModeLikelihood}; `coverage`: {variable: the share of its points in a kept mode}; `skipped`: the factors left
    out as unsupported."""
    variables: list
    modes: dict
    best: dict
    best_points: dict
    best_logscore: float
    logZ: float
    best_weight: float
    combos: np.ndarray
    logscores: np.ndarray
    weights: np.ndarray
    tables: dict
    coverage: dict
    skipped: list = field(default_factory=list)


def score_terms(tables):
    """{factor: FactorModeLikelihood} -> the terms of `joint_modes_from_tables`"""
    terms = []
    for r in tables.values():
        items = [((a,), t[:, 0]) if b is None else ((a, b), t) for (a, b), t in zip(r.variables, r.tables)]
        terms.append(MultihypoTerm(r.hypo_prior, items) if r.hypotheses else items[0])
    return terms


def joint_from_tables(modes, tables, skipped, maxModes=MAXK, cap=2**22, enumerate_up_to=4096):
    """the modes of the variables and the tables of the factors -> JointModes"""
    used = sorted({v for r in tables.values() for pair in r.variables for v in pair if v is not None}, key=_natural)
    K = {v: kept_modes(modes[v], maxModes) for v in used}
    sol = joint_modes_from_tables(K, score_terms(tables), cap, enumerate_up_to)
    cov = {}
    for r in tables.values():
        cov.update(r.coverage)
    pts = {v: (np.array(modes[v].modes[k]) if k < len(modes[v].modes) else None) for v, k in sol.best.items()}
    return JointModes(sol.variables, {v: modes[v] for v in used}, sol.best, pts, sol.best_logscore, sol.logZ, sol.best_weight, sol.combos,
                      sol.logscores, sol.weights, dict(tables), {v: cov[v] for v in used}, list(skipped))


def jointModes(fg, labels=None, maxModes=MAXK, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER,
               merge=abi.MODES_MERGE, backend=None):
    """The joint hypothesis of the graph under the current beliefs: the modes of every variable the factors `labels` (default: every
    factor; the unsupported ones go to `.skipped`, a named one is a ValueError) touch, their mode-by-mode likelihood tables and the
    exact maximum and normaliser of the joint score -> JointModes.  On a HIP backend the beliefs are written once, then one
    run_modes launch and one table launch; otherwise numpy."""
    maxModes = _check_max_modes(maxModes)
    kw = _modes._options(bwScale, tol, maxIter, merge)
    plans, skipped = likelihood.plan_factors(fg, labels, skip_unsupported=labels is None)
    modes, res = _tables_of(fg, plans, None, maxModes, backend, kw)
    return joint_from_tables(modes, {p.label: res[p.label] for p in plans}, skipped, maxModes)
