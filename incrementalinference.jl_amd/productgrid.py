"""Local products on a grid: the product of the messages a variable's factors send it, without particles for the variable itself.

Every other query of this package describes a belief as it stands.  This one says what the belief SHOULD be: the reference's
`localProduct(fg, :x5)` -- one Gibbs update, the core operation of the solver -- multiplies the factors' messages with N particles,
a fitted bandwidth per proposal and a multiscale Gibbs sampler.  Here the variable's clouds are replaced by a regular grid over its
coordinates; every factor's message is the closed-form measurement density at the cell, summed over the neighbour's cloud; the logs
are added and normalised by quadrature.  It is what one update of x5 would return with infinitely many particles and no kernel
smoothing, given the same neighbour clouds: a yardstick for the product, the bandwidths and the sampler that shares no code with
them, a noise-free picture of a pose's conditional posterior, and its evidence `logZ`.

The definition ("Local products on a grid"; include/nbp.h, nbp_run_product_grid; DEFINED here and unpinned):

  cell       x = (lo[a] + float(k_a) * step[a])_a, one axis per coordinate of the manifold (SE(2): x, y, theta), row-major
  e_jc(x)    `likelihood.pair_terms` with x in role a and the neighbour's u_j in role b (role 0), or the other way round (role 1);
             a prior: e_c(x) alone
  log m(x)   M = max_jc e_jc;  S_c = sum_j exp(e_jc - M), j in order, below exp(-700) zero;  S = sum_c S_c;  (M + log S) - log n
  group      the hypotheses of a multihypo factor whose certain variable this is: t_k = log p_k + log m_k(x), one item: l = t_0,
             more: a running max-shift in item order (`_group_step`)
  L(x)       sum_g l_g(x) in list order from 0;  logmax, argmax (lowest index),
             logZ = (logmax + log sum exp(L - logmax)) + sum_a log step[a]  (an axis of one point is a slice and adds nothing)

No bandwidth enters a value; the variable's own belief is read for the automatic extent alone (`marginalGrid`'s rule per axis).
What is left out (listed in `.skipped`, a ValueError when named): factors where the variable is a FRACTIONAL variable of a multihypo
(their message has a flat part without a normaliser) and everything `likelihood.factor_items` refuses (message and pass-through
priors, tables, KDE measurements); `nullhypo` is ignored.

On a HIP backend every grid of a call is one launch sequence (`HipBackend.run_product_grid`, csrc/nbp_productgrid.h);
`product_grid_numpy` restates the definition on the host in the same order of operations and serves tests, readers and callers
without such a backend -- never as a fallback on a device failure."""
import math
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .beliefquery import _manifold, _staged, _wrap
from .likelihood import _UNARY, _coords, block_sum_numpy, factor_items, pair_terms, shifted_exp
from .marginal import grid_extent_numpy
from .ppe import _circular, _natural

_BLOCK = 1 << 21  # pair terms per block of cells in the restatement


# ------------------------------------------------------------------------------------------------
# the definition on the host
# ------------------------------------------------------------------------------------------------
def _sizes(manifold, n):
    D = abi.MANIFOLD_DIM[manifold]
    n = [int(v) for v in np.atleast_1d(n)]
    n = n * D if len(n) == 1 else n
    if len(n) != D:
        raise ValueError(f"product grid: one size per coordinate ({D}), got {n}")
    return n


def grid_axes(extent, n):
    """the coordinate vectors of a grid: point k of axis a = lo_a + float(k) * step_a; extent = (lo0, step0, lo1, step1, ...)"""
    return [np.float64(extent[2 * a]) + np.arange(n[a], dtype=np.float64) * np.float64(extent[2 * a + 1]) for a in range(len(n))]


def grid_cells(axes):
    """every cell of the grid as a row of coordinates, row-major with coordinate 0 slowest -> (cells, D)"""
    return np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)


def product_extent_numpy(manifold, X, bw, n, margin=abi.PGRID_MARGIN):
    """the automatic extent: `marginal.grid_extent_numpy`'s rule on every coordinate of the manifold -> [lo0, step0, .. ] (2 D)"""
    D = abi.MANIFOLD_DIM[manifold]
    n = _sizes(manifold, n)
    ext = np.zeros(2 * D)
    for a in range(D):
        ext[2 * a:2 * a + 2] = grid_extent_numpy(manifold, X, bw, [a], [n[a]], margin)[:2]
    return ext


def message_numpy(desc, role, cells, other, dtype=np.float64):
    """log m(x) of one item at the rows of `cells` (tangent coordinates): other = the host points of the other variable (n x P),
    None for a prior"""
    T = dtype
    out = np.empty(cells.shape[0], dtype=T)
    unary = desc.kind in _UNARY
    nb = 1 if unary else _coords(desc.manifold, other, T).shape[0]
    blk = max(1, _BLOCK // max(nb, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k0 in range(0, cells.shape[0], blk):
            x = cells[k0:k0 + blk]
            if unary:
                e = pair_terms(desc, x, None, T)
            elif role == 0:
                e = pair_terms(desc, x, other, T)
            else:
                e = [v.T for v in pair_terms(desc, other, x, T)]
            Mx = e[0].max(axis=1)
            for v in e[1:]:
                Mx = np.maximum(Mx, v.max(axis=1))
            S = np.zeros(x.shape[0], dtype=T)
            for v in e:
                S = S + np.cumsum(shifted_exp(v - Mx[:, None], T), axis=1)[:, -1]  # (a cumulative sum along j: the running sum in j order)
            out[k0:k0 + blk] = np.where(Mx > -np.inf, (Mx + np.log(S)) - np.log(T(nb)), T(-np.inf))
    return out


def _group_step(gm, gs, t, T):
    """one step of the running max-shift of a group: (mx, s) and the next t_k -> (mx, s)"""
    with np.errstate(invalid="ignore"):
        up = t > gm
        ex = shifted_exp(np.where(up, gm - t, t - gm), T)
        s_up = np.where(gm > -np.inf, gs * ex, T(0)) + T(1)
        s_in = np.where(t > -np.inf, gs + ex, gs)
    return np.where(up, t, gm), np.where(up, s_up, s_in)


def normalise_numpy(L, n, step, dtype=np.float64):
    """the record of one grid from its flat L: (logZ, logmax, argmax) -- lane t of 256 adds the cells t, t + 256, .. in order, the lanes
    are added as libnbp's block sum adds them"""
    T = dtype
    L = np.asarray(L, dtype=T).reshape(-1)
    logmax = np.fmax.reduce(L) if L.size else T(-np.inf)
    if not logmax > -np.inf:
        return T(-np.inf), T(-np.inf), -1
    argmax = int(np.flatnonzero(L == logmax)[0])
    with np.errstate(invalid="ignore"):
        w = shifted_exp(L - logmax, T)
    pad = np.zeros(-(-w.size // abi.PGRID_CHUNK) * abi.PGRID_CHUNK, dtype=T)
    pad[:w.size] = w
    Z = block_sum_numpy(np.cumsum(pad.reshape(-1, abi.PGRID_CHUNK), axis=0)[-1])
    ls = T(0)
    for a in range(len(n)):
        if n[a] > 1:
            ls = ls + np.log(T(step[a]))
    return (logmax + np.log(Z)) + ls, logmax, argmax


def product_grid_numpy(manifold, n, extent, items, dtype=np.float64):
    """the definition on the host, in the arithmetic `dtype` (np.longdouble: the measure of a case's conditioning).  n: the cells per
    coordinate; extent = (lo0, step0, lo1, step1, ..) as used; items = [(desc, role, other, group, log_prior)]: an
    abi.LikelihoodDesc (its slots are not read), the role of the grid's variable, the host points of the other variable (n x P; None
    for a prior), the group (non-decreasing) and the log prior -> (logp of shape n, logZ, logmax, argmax)"""
    T = dtype
    n = _sizes(manifold, n)
    extent = np.asarray(extent, dtype=np.float64).reshape(-1)
    cells = grid_cells(grid_axes(extent, n))
    L = np.zeros(cells.shape[0], dtype=T)
    gm = gs = t0 = None
    gc = 0
    for i, (desc, role, other, group, log_prior) in enumerate(items):
        if desc.manifold != manifold:
            raise ValueError(f"product grid: item {i} lies on another manifold than the grid")
        if role not in (0, 1) or (desc.kind in _UNARY and (role == 1 or other is not None)):
            raise ValueError(f"product grid: item {i}: role outside 0 / 1, or a unary item with a role 1 or another variable")
        if i and group < items[i - 1][3]:
            raise ValueError(f"product grid: item {i}: groups must not decrease along the list")
        if math.isnan(log_prior) or log_prior == math.inf:
            raise ValueError(f"product grid: item {i}: log_prior is NaN or +inf")
        t = T(log_prior) + message_numpy(desc, role, cells, other, T)
        if i == 0 or items[i - 1][3] != group:
            gm, gs, gc, t0 = np.full(L.shape, -np.inf, dtype=T), np.zeros(L.shape, dtype=T), 0, t
        gc += 1
        gm, gs = _group_step(gm, gs, t, T)
        if i == len(items) - 1 or items[i + 1][3] != group:
            with np.errstate(divide="ignore", invalid="ignore"):
                L = L + (t0 if gc == 1 else np.where(gm > -np.inf, gm + np.log(gs), T(-np.inf)))
    logZ, logmax, argmax = normalise_numpy(L, n, extent[1::2], T)
    return L.reshape(n), logZ, logmax, argmax


# ------------------------------------------------------------------------------------------------
# the result
# ------------------------------------------------------------------------------------------------
def _logsumexp_axes(a, axes):
    if not axes:
        return a
    m = a.max(axis=axes, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.log(np.exp(a - np.where(m > -np.inf, m, 0.0)).sum(axis=axes, keepdims=True)) + m
    return np.squeeze(np.where(m > -np.inf, s, -np.inf), axis=axes)


@dataclass
class ProductGrid:
    """L(x) of one variable on its grid.  logp: shape n, coordinate 0 slowest (unnormalised: `density()` divides by the evidence);
    axes: the coordinate vectors; extent: (lo0, step0, lo1, step1, ..) as used; logZ: the log evidence by quadrature; logmax and
    argmax: the largest cell (flat index, -1 where every cell is -inf) and `point` its coordinates; factors: the labels that
    entered, in list order; skipped: the labels left out as unsupported"""
    manifold: int
    logp: np.ndarray
    axes: list
    extent: np.ndarray
    logZ: float
    logmax: float
    argmax: int
    point: np.ndarray
    factors: list = field(default_factory=list)
    skipped: list = field(default_factory=list)

    def density(self):
        """exp(logp - logZ): integrates to 1 by the grid's own quadrature"""
        with np.errstate(invalid="ignore"):
            return np.exp(self.logp - self.logZ)

    def _logsteps(self, axes):
        return sum(math.log(self.extent[2 * a + 1]) for a in axes if self.logp.shape[a] > 1)

    def marginal(self, dims):
        """the log of the normalised marginal density on the 1-BASED coordinates `dims` (like `marginalGrid`), in that order: a
        logsumexp over the dropped axes plus their log steps.  Host arithmetic."""
        dims = [int(d) - 1 for d in np.atleast_1d(dims)]
        D = self.logp.ndim
        if not dims or len(set(dims)) != len(dims) or min(dims) < 0 or max(dims) >= D:
            raise ValueError(f"marginal: distinct 1-based coordinates within 1..{D}")
        drop = tuple(a for a in range(D) if a not in dims)
        m = _logsumexp_axes(self.logp, drop) + self._logsteps(drop) - self.logZ
        kept = [a for a in range(D) if a in dims]
        return np.transpose(m, [kept.index(d) for d in dims])

    def moments(self):
        """(mean[D], cov[D, D]) under the grid; circular coordinates about `point` (deviations wrapped, the mean wrapped back)"""
        D = self.logp.ndim
        if self.argmax < 0:
            return np.full(D, np.nan), np.full((D, D), np.nan)
        w = np.exp(self.logp - self.logmax).reshape(-1)
        w = w / w.sum()
        X = grid_cells(self.axes)
        circ = _circular(self.manifold)
        dev = X - self.point[None, :]
        for a in range(D):
            if circ[a]:
                dev[:, a] = _wrap(dev[:, a])
        m = w @ dev
        dev = dev - m[None, :]
        mean = self.point + m
        for a in range(D):
            if circ[a]:
                mean[a] = _wrap(mean[a])
        return mean, (dev * w[:, None]).T @ dev


def _result(manifold, n, logp, rec, ext, factors, skipped):
    D = abi.MANIFOLD_DIM[manifold]
    ext = np.array(ext, dtype=np.float64).reshape(-1)[:2 * D]
    axes = grid_axes(ext, n)
    argmax = int(rec[2])
    point = np.array([axes[a][k] for a, k in enumerate(np.unravel_index(argmax, n))]) if argmax >= 0 else np.full(D, np.nan)
    return ProductGrid(manifold, np.asarray(logp, dtype=np.float64).reshape(n), axes, ext, float(rec[0]), float(rec[1]), argmax, point,
                       list(factors), list(skipped))


# ------------------------------------------------------------------------------------------------
# a variable of a graph as items
# ------------------------------------------------------------------------------------------------
@dataclass
class _VarPlan:
    label: str
    manifold: int
    items: list     # (desc, role, label of the other variable or None, group, log_prior)
    factors: list
    skipped: list
    roles: list     # the variables whose beliefs the plan reads, as one-element tuples (`SolveSession._query_resident_factors`)


def variable_items(fg, label, factors=None):
    """`likelihood.factor_items` turned from "by factor" to "by variable": the messages the factors `factors` (default: every factor
    of the variable, natural order; the unsupported ones go to `.skipped`) send the variable `label` -> _VarPlan.  A named factor
    that is unsupported, or that does not touch the variable, is a ValueError."""
    man = _manifold(fg.getVariable(label).varType)
    named = factors is not None
    mine = sorted(fg.ls(label), key=_natural)
    flist = list(factors) if named else mine
    items, used, skipped = [], [], []
    for f in flist:
        try:
            if f not in mine:
                raise ValueError(f"localProductGrid: factor {f} does not touch variable {label}")
            plan = factor_items(fg, f)
            if label in plan.hypotheses:
                raise ValueError(f"localProductGrid: factor {f}: {label} is a fractional variable of the multihypo factor: its message "
                                 "has a flat part without a normaliser")
            new = []
            for k, (d, (a, b)) in enumerate(zip(plan.descs, plan.roles)):
                if d.manifold != man or (a == label) == (b == label):
                    raise ValueError(f"localProductGrid: factor {f}: {label} does not fill exactly one role on its own manifold")
                lp = math.log(plan.prior[k]) if plan.hypotheses else 0.0
                new.append((d, 0 if a == label else 1, b if a == label else a, len(used), lp))
        except ValueError:
            if named:
                raise
            skipped.append(f)
            continue
        items += new
        used.append(f)
    others = []
    for it in items:
        if it[2] is not None and it[2] not in others and it[2] != label:
            others.append(it[2])
    return _VarPlan(label, man, items, used, skipped, [(v,) for v in [label] + others])


def _extent_of(extent, label):
    e = extent.get(label) if isinstance(extent, dict) else extent
    return None if e is None else np.asarray(e, dtype=np.float64).reshape(-1)


def _grid_desc(plan, n, extent, margin, place, first_item):
    D = abi.MANIFOLD_DIM[plan.manifold]
    g = abi.ProductGridDesc(manifold=plan.manifold, slot=place[plan.label], margin=float(margin), first_item=first_item, n_items=len(plan.items))
    g.n[:] = n + [1] * (3 - D)
    if extent is None:
        g.flags = abi.PGRID_AUTO_EXTENT
    else:
        if extent.size != 2 * D:
            raise ValueError("an extent is (lo, step) per coordinate")
        for a in range(D):
            g.lo[a], g.step[a] = extent[2 * a], extent[2 * a + 1]
    return g


def run_plans(be, plans, place, n=64, extent=None, margin=abi.PGRID_MARGIN):
    """ONE run_product_grid for every grid of every plan, the beliefs read in the slots `place` names -> {label: ProductGrid}"""
    grids, items, sizes = [], [], []
    for p in plans:
        sizes.append(_sizes(p.manifold, n))
        grids.append(_grid_desc(p, sizes[-1], _extent_of(extent, p.label), margin, place, len(items)))
        for d, role, other, group, lp in p.items:
            it = abi.ProductItem(role=role, other=-1 if other is None else place[other], group=group, log_prior=lp)
            it.lik = d
            items.append(it)
    if not grids:
        return {}
    logp, rec, ext = be.run_product_grid(grids, items)
    return {p.label: _result(p.manifold, sizes[i], logp[i], (rec["logZ"][i], rec["logmax"][i], rec["argmax"][i]), ext[i], p.factors, p.skipped)
            for i, p in enumerate(plans)}


def _host_plan(fg, p, n, extent, margin, dtype=np.float64):
    v = fg.getVariable(p.label)
    nn = _sizes(p.manifold, n)
    ext = _extent_of(extent, p.label)
    if ext is None:
        ext = product_extent_numpy(p.manifold, _coords(p.manifold, v.val, np.float64), v.bw, nn, margin)
    items = [(d, role, None if other is None else fg.getVariable(other).val, group, lp) for d, role, other, group, lp in p.items]
    logp, logZ, logmax, argmax = product_grid_numpy(p.manifold, nn, ext, items, dtype)
    return _result(p.manifold, nn, logp, (logZ, logmax, argmax), ext, p.factors, p.skipped)


def localProductGridAll(fg, labels=None, n=64, extent=None, margin=abi.PGRID_MARGIN, backend=None):
    """-> {label: ProductGrid} of the variables `labels` (default: every variable) in natural order.  n: the cells per coordinate (a
    scalar: the same on every axis); extent: (lo0, step0, lo1, step1, ..) for all, a dict {label: extent}, or None for the automatic
    extent with `margin` bandwidths around each variable's own belief.  On a HIP backend the beliefs are written once and ONE
    run_product_grid serves every grid; otherwise numpy."""
    labels = sorted(fg.ls(), key=_natural) if labels is None else list(labels)
    plans = [variable_items(fg, v) for v in labels]
    names = []
    for p in plans:
        names += [r[0] for r in p.roles if r[0] not in names]
    with _staged(fg, names, backend, "run_product_grid") as (be, place):
        if be is None:
            return {p.label: _host_plan(fg, p, n, extent, margin) for p in plans}
        return run_plans(be, plans, place, n, extent, margin)


def localProductGrid(fg, label, n=64, extent=None, margin=abi.PGRID_MARGIN, factors=None, backend=None):
    """The product of the messages the factors of variable `label` send it, on a regular grid over its coordinates -> ProductGrid:
    the grid twin of the reference's `localProduct(fg, label)`.  n, extent, margin and backend as in `localProductGridAll`;
    factors: the factor labels that enter, in this order (default: every supported factor of the variable in natural order, the
    others listed in `.skipped`); naming an unsupported factor is a ValueError."""
    p = variable_items(fg, label, factors)
    with _staged(fg, [r[0] for r in p.roles], backend, "run_product_grid") as (be, place):
        if be is None:
            return _host_plan(fg, p, n, extent, margin)
        return run_plans(be, [p], place, n, extent, margin)[label]
