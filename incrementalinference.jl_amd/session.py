"""Solve sessions: one device context that outlives a solve, with the beliefs resident between incremental solves.

`solveTree(fg, oldtree=tree)` makes a context, uploads every belief, runs, reads every updated belief back and tears the
context down -- and graph initialisation does the same once more in a context of its own.  On the loop a SLAM front end runs
(solve, add a pose, solve again) that fixed cost is paid for the whole graph at every step.  A `SolveSession` keeps ONE backend
instance; both schedule compilers put the belief of variable v in slot main[v] = its place in the add order, and main[v] is
written by v's frontal clique alone, so the posteriors of the last solve lie exactly where the next program reads its inputs.
What travels is what changed: new variables and host edits go up, the beliefs a program updated come down.  No new kernel: the
hot path is host traffic that no longer happens."""
import time

import numpy as np

from . import abi, bayestree
from .ppe import MeanMaxPPE
from .solver import (TreeProgram, _initialised_subgraph, _make_backend, _refuse_joint_recycling, _runs_on_libnbp,
                     _untouched_variables, initStages, passthrough_factors, setValKDE, write_densities)


class _Resident:
    """what the device holds in one variable slot: `label`'s belief, equal to the host arrays `val` and `bw` (kept referenced,
    so that their identity can never be taken by another array) -- or, `pending`, newer than the host copy"""
    __slots__ = ("label", "val", "bw", "pending")

    def __init__(self, label, val, bw, pending=False):
        self.label, self.val, self.bw, self.pending = label, val, bw, pending


def _density_slots(fg):
    return {f: fg.getFactor(f).fnc.slot for f in passthrough_factors(fg)}


def _place_densities(fg, slots):
    for f, s in slots.items():
        fg.getFactor(f).fnc.slot = s


class SolveSession:
    """SolveSession(fg, backend=None, reserve=0): incremental solves of a growing graph in one device context.

    `ses.solve(...)` is `solveTree(fg, oldtree=ses.tree, ...)` in every respect a caller can observe -- fifoFreeze, graph
    initialisation, tree, clique recycling against the previous tree, up pass, down pass, posteriors, solvedCount, PPE and
    clique statuses, with the same seeds -- but the beliefs stay on the device between solves.  `backend`: a factory
    make(N, n_slots, side_ints=0), or None for HipBackend.  `reserve`: slots to start with (the context holds
    max(reserve, 1.5 x the first solve's need); a solve that needs more replaces it by one of 1.5 x that need and uploads
    everything again -- the policy looks at slot counts only, so it is the same on every backend).

    Residency.  For every variable slot the session knows whose belief the device holds and which host arrays (`var.val`,
    `var.bw`, by object identity) it equals.  Before a program runs, whatever is missing, stale or displaced is uploaded in one
    batch; afterwards only the beliefs the program updated are read back, in one batch, and the arrays that come back are the
    new tokens.  `setValKDE` / `initVariable` assign fresh arrays, so edits between solves are seen.  An edit IN PLACE
    (`fg.getVal("x3")[:] = ...`) is not: call `ses.invalidate("x3")`.  Frozen, recycled and otherwise untouched variables are
    neither uploaded nor read, and keep the `ppe` they have.  The beliefs graph initialisation produces stay on the device for
    the tree program and reach the host with its results.

    What "the same as solveTree" means.  Euclid(1-3) and Circular: bit-identical to `solveTree(oldtree=...)` with the same
    seeds (a slot stores these coordinates as the host sees them).  SE(2): a slot stores the heading as theta, the host sees
    cos and sin, and a write converts back with atan2 -- a belief that stayed resident can differ from its host round trip in
    the last bit.  There the session is its own definition: bit-identical between the oracle backend and libnbp, held to the
    reference's bands, not compared bit for bit with `solveTree`.

    When a solve raises, the residency table is cleared (the host copy wins at the next solve), variables graph initialisation
    had reached in that solve but whose beliefs never came back are uninitialised again, and the context stays usable.

    `ses.tree`: the tree of the last solve (None before the first).  `ses.stats`: uploads, readbacks (beliefs, cumulative),
    contexts, resyncs (table cleared: growth or renumbering), solves, slots (the last solve's need), capacity, and under
    "last" the uploads, readbacks and resyncs of the last solve."""

    def __init__(self, fg, backend=None, reserve=0):
        if backend is not None and hasattr(backend, "slot_write"):
            raise TypeError("SolveSession takes a backend factory (or None), not an instance: it sizes the context itself")
        self.fg, self.backend, self.reserve = fg, backend, int(reserve)
        self.tree = None
        self._be = None
        self._closed = False
        self._table = {}    # variable slot -> _Resident
        self._labels = []   # the labels of the subgraph the last solve worked on, in slot order
        self.stats = {"uploads": 0, "readbacks": 0, "contexts": 0, "resyncs": 0, "solves": 0, "slots": 0, "capacity": 0,
                      "last": {"uploads": 0, "readbacks": 0, "resyncs": 0}}

    # ---- life cycle ---------------------------------------------------------------------------------------------------
    def close(self):
        """closes the context (programs go before it); harmless when repeated"""
        self._closed = True
        self._table.clear()
        be, self._be = self._be, None
        if be is not None:
            be.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def invalidate(self, *labels):
        """the host copy of these variables (no labels: of all) wins at the next solve; their stored PPE goes too"""
        if not labels:
            self._table.clear()
        for s in [s for s, e in self._table.items() if e.label in labels]:
            del self._table[s]
        for v in (labels or self.fg.ls()):
            if v in self.fg.variables:
                self.fg.getVariable(v).ppe = None

    # ---- the context and the table --------------------------------------------------------------------------------------
    def _resync(self):
        self._table.clear()
        self.stats["resyncs"] += 1
        self.stats["last"]["resyncs"] += 1

    def _ensure_capacity(self, needed):
        st, N = self.stats, self.fg.solverParams.N
        if self._be is not None and needed <= st["capacity"] and self._be.N == N:
            return
        grown = self._be is not None
        if grown:
            self._be.close()
            self._be = None
            self._resync()
        cap = needed + needed // 2 if grown else max(self.reserve, needed + needed // 2)
        self._be, _ = _make_backend(self.backend, N, cap)
        st["capacity"] = cap
        st["contexts"] += 1

    def _upload(self, graph, expected, V):
        """make the device hold what a program with `V` variable slots expects: expected = [(label, slot)]"""
        for s in [s for s in self._table if s >= V]:  # scratch of this program
            del self._table[s]
        todo = []
        for label, slot in expected:
            var, e = graph.getVariable(label), self._table.get(slot)
            if e is not None and e.label == label and (e.pending or (e.val is var.val and e.bw is var.bw)):
                continue
            todo.append((label, slot, var))
        if not todo:
            return
        be = self._be
        mans = [var.varType.manifold for _, _, var in todo]
        if getattr(be, "beliefs_write", None) is not None:
            be.beliefs_write([s for _, s, _ in todo], mans, [(var.val, var.bw, None) for _, _, var in todo])
        else:
            for (_, slot, var), man in zip(todo, mans):
                be.belief_write(slot, man, var.val, var.bw)
        for label, slot, var in todo:
            self._table[slot] = _Resident(label, var.val, var.bw)
        self.stats["uploads"] += len(todo)
        self.stats["last"]["uploads"] += len(todo)

    def _readback(self, graph, wanted):
        """the beliefs of wanted = [(label, slot)] -> the host graph (setValKDE); the new arrays become the table's tokens"""
        if not wanted:
            return
        be = self._be
        mans = [graph.getVariable(v).varType.manifold for v, _ in wanted]
        if getattr(be, "beliefs_read", None) is not None:
            got = be.beliefs_read([s for _, s in wanted], mans)
        else:
            got = [be.belief_read(s, m) for (_, s), m in zip(wanted, mans)]
        for (v, slot), (pts, bw, _) in zip(wanted, got):
            setValKDE(graph, v, pts, bw, True)
            var = graph.getVariable(v)
            self._table[slot] = _Resident(v, var.val, var.bw)
        self.stats["readbacks"] += len(wanted)
        self.stats["last"]["readbacks"] += len(wanted)

    # ---- statistics of the resident beliefs ------------------------------------------------------------------------------
    def _query_resident(self, labels, method, args, pick, host, call=None):
        """One query of the variables' current beliefs -> {label: result} in the order of `labels` (default: every variable the
        last solve worked on).  On a backend that has `method`, the beliefs the residency table holds as current are read where
        they lie, in ONE call `method(*args(here, place))` -- here: the labels that have a slot, place: label -> slot -- and
        `pick(result, i, label)` is what that call holds for here[i]: no belief travels and `stats` does not move.  A belief that
        is not resident (edited on the host since, or invalidated) goes up first by the session's upload path and is counted as
        an upload.  `host(label, **kw)` is the same query on the host copy: for every label where there is no context or the
        backend lacks `method`, and with backend=self.backend for a variable that has no slot in the session's context (never
        part of a solve).  call: a query of several launches, `call(backend, *args(here, place))` in place of the one method."""
        if self._closed:
            raise RuntimeError("this SolveSession is closed")
        labels = list(self._labels if labels is None else labels)
        be = self._be
        place = {v: i for i, v in enumerate(self._labels)}
        if be is None or getattr(be, method, None) is None:
            return {v: host(v) for v in labels}
        out = {}
        here = [v for v in labels if v in place]
        if here:
            try:
                self._upload(self.fg, [(v, place[v]) for v in here], len(self._labels))
                res = call(be, *args(here, place)) if call is not None else getattr(be, method)(*args(here, place))
            except BaseException:
                self._table.clear()  # the device state is unknown: the host copy wins
                raise
            for i, v in enumerate(here):
                out[v] = pick(res, i, v)
        for v in labels:
            if v not in place:
                out[v] = host(v, backend=self.backend)
        return {v: out[v] for v in labels}

    def calcMeanCovar(self, labels=None):
        """calcMeanCovar (VariableStatistics.jl:39-44) of the variables' current beliefs -> {label: (mu[D], Sigma[D, D])}, served
        by ONE `run_meancov` launch where libnbp holds the beliefs (`_query_resident`); on the host copy,
        `beliefstats.calcMeanCovar`."""
        from . import beliefstats
        var = self.fg.getVariable

        def pick(res, i, v):
            D = var(v).varType.dim
            return res[0][i, :D].copy(), res[1][i, :D, :D].copy()
        return self._query_resident(labels, "run_meancov",
                                    lambda here, place: ([place[v] for v in here], [var(v).varType.manifold for v in here]), pick,
                                    lambda v, **kw: beliefstats.calcMeanCovar(self.fg, v, **kw))

    def marginalGrid(self, labels=None, dims=(1,), n=64, margin=4.0):
        """The marginal densities of the variables' current beliefs on regular grids with the automatic extent (marginal.py) ->
        {label: (grid, axes)}.  dims: one or two coordinates, 1-BASED like the reference's `partial`; n: points per axis (a scalar:
        the same on both); labels: default every variable the last solve worked on whose manifold has the coordinates `dims`.
        Served by ONE `run_marginal_grid` where libnbp holds the beliefs (`_query_resident`); on the host copy,
        `marginal.marginalGrid`."""
        from . import marginal
        dims = tuple(int(d) for d in (dims if hasattr(dims, "__len__") else (dims,)))
        nn = [int(v) for v in (n if hasattr(n, "__len__") else (n,))]
        nn = nn * len(dims) if len(nn) == 1 else nn
        var = self.fg.getVariable
        if labels is None:  # (a generator: read behind the closed check)
            labels = (v for v in self._labels if var(v).varType.dim >= max(dims))
        return self._query_resident(labels, "run_marginal_grid",
                                    lambda here, place: ([(place[v], var(v).varType.manifold, [d - 1 for d in dims], nn, None, margin)
                                                          for v in here], True),
                                    lambda res, i, v: (res[0][i].copy(), marginal.grid_axes(res[1][i], nn)),
                                    lambda v, **kw: marginal.marginalGrid(self.fg, v, dims, nn, None, margin, **kw))

    def getBeliefModes(self, labels=None, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER, merge=abi.MODES_MERGE):
        """The modes of the variables' current beliefs (modes.py: mean-shift from every point, merged and ranked) ->
        {label: BeliefModes}, served by ONE `run_modes` launch where libnbp holds the beliefs (`_query_resident`); on the host
        copy, `modes.getBeliefModes`."""
        from . import modes
        kw = modes._options(bwScale, tol, maxIter, merge)
        var = self.fg.getVariable
        return self._query_resident(labels, "run_modes",
                                    lambda here, place: ([place[v] for v in here], [var(v).varType.manifold for v in here], *kw.values()),
                                    lambda res, i, v: modes.modes_from_records(var(v).varType.manifold, *(r[i] for r in res)),
                                    lambda v, **k: modes.getBeliefModes(self.fg, v, bwScale, tol, maxIter, merge, **k))

    def _query_resident_factors(self, plans, method, run, host):
        """The factor-shaped sibling of `_query_resident`: one query of factors, each reading the current beliefs of SEVERAL
        variables -> {factor label: result}.  plans: objects with `.label` and `.roles` (tuples of variable labels, None for an
        empty role).  On a backend that has `method`, the factors whose variables all have a slot are served where the beliefs
        lie by ONE call `run(be, plans_here, place)` -- place: variable label -> slot --: no belief travels and `stats` does not
        move; a belief that is not resident goes up first by the session's upload path and is counted as an upload.
        `host(plan, **kw)` is the same query on the host copy: for every factor where there is no context or the backend lacks
        `method`, and with backend=self.backend for a factor with a variable that has no slot in the session's context."""
        if self._closed:
            raise RuntimeError("this SolveSession is closed")
        be = self._be
        if be is None or getattr(be, method, None) is None:
            return {p.label: host(p) for p in plans}
        place = {v: i for i, v in enumerate(self._labels)}
        need = lambda p: [v for r in p.roles for v in r if v is not None]  # noqa: E731
        here = [p for p in plans if all(v in place for v in need(p))]
        out = {}
        if here:
            want = []
            for p in here:
                want += [v for v in need(p) if v not in want]
            try:
                self._upload(self.fg, [(v, place[v]) for v in want], len(self._labels))
                out.update(run(be, here, place))
            except BaseException:
                self._table.clear()  # the device state is unknown: the host copy wins
                raise
        for p in plans:
            if p.label not in out:
                out[p.label] = host(p, backend=self.backend)
        return {p.label: out[p.label] for p in plans}

    def factorLikelihoods(self, labels=None):
        """The likelihood of the factors `labels` (default: every factor of the graph, the unsupported ones listed in the result's
        `.skipped`; a named unsupported factor is a ValueError) under the variables' current beliefs (likelihood.py) ->
        FactorLikelihoods {label: FactorLikelihood} in natural order, served by ONE `run_factor_likelihood` launch for every item
        of every factor where libnbp holds the beliefs (`_query_resident_factors`); on the host copy,
        `likelihood.factorLikelihood`."""
        from . import likelihood
        plans, skipped = likelihood.plan_factors(self.fg, labels, skip_unsupported=labels is None)
        res = self._query_resident_factors(plans, "run_factor_likelihood", likelihood.run_plans,
                                           lambda p, **kw: likelihood.factorLikelihood(self.fg, p.label, **kw))
        return likelihood.FactorLikelihoods(res.items(), skipped=skipped)

    def localProductGrids(self, labels=None, n=64, extent=None, margin=abi.PGRID_MARGIN):
        """The product of the messages every variable's factors send it, on a grid per variable (productgrid.py) ->
        {label: ProductGrid} in natural order.  labels: default every variable the last solve worked on; n, extent and margin as in
        `productgrid.localProductGridAll`.  Served by ONE `run_product_grid` for every grid where libnbp holds the beliefs
        (`_query_resident_factors`: a variable and its neighbours are one plan): no belief travels and `stats` does not move; on the
        host copy, `productgrid.localProductGrid`."""
        from . import productgrid
        if labels is None:
            labels = list(self._labels) if self._labels else self.fg.ls()
        plans = [productgrid.variable_items(self.fg, v) for v in sorted(labels, key=productgrid._natural)]
        return self._query_resident_factors(plans, "run_product_grid",
                                            lambda be, here, place: productgrid.run_plans(be, here, place, n, extent, margin),
                                            lambda p, **kw: productgrid.localProductGrid(self.fg, p.label, n, extent, margin, **kw))

    def jointModes(self, labels=None, maxModes=abi.MAXK, bwScale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, maxIter=abi.MODES_MAX_ITER,
                   merge=abi.MODES_MERGE):
        """The joint hypothesis of the graph under the variables' current beliefs (jointmodes.py): which mode of one variable
        belongs with which mode of another, and the weight of every combination -> JointModes.  labels: the factors that enter
        (default: every factor, the unsupported ones listed in `.skipped`; a named unsupported factor is a ValueError).  Where
        libnbp holds the beliefs, the modes come from ONE `run_modes` launch (`getBeliefModes` through `_query_resident`) and the
        tables from ONE `run_factor_mode_likelihood` launch (`_query_resident_factors`): no belief travels and `stats` does not
        move.  On the host copy, `jointmodes.jointModes`."""
        from . import jointmodes, likelihood
        maxModes = jointmodes._check_max_modes(maxModes)
        plans, skipped = likelihood.plan_factors(self.fg, labels, skip_unsupported=labels is None)
        modes = self.getBeliefModes(jointmodes._plan_variables(plans), bwScale, tol, maxIter, merge)
        res = self._query_resident_factors(plans, "run_factor_mode_likelihood",
                                           lambda be, here, place: jointmodes.run_mode_plans(be, here, place, modes, maxModes),
                                           lambda p, **kw: jointmodes.factorModeLikelihood(self.fg, p.label, modes, maxModes, **kw))
        return jointmodes.joint_from_tables(modes, res, skipped, maxModes)

    def _device_labels(self, labels, what, method, name):
        """the labels of a query that has no host route: all of them must have a slot in the session's context, since the query
        is computed where the beliefs lie"""
        if self._closed:
            raise RuntimeError("this SolveSession is closed")
        labels = list(self._labels if labels is None else labels)
        if self._be is None or getattr(self._be, method, None) is None:
            raise ValueError(f"{what}: {name} are computed by libnbp, and this session's backend has no such entry point")
        missing = [v for v in labels if v not in self._labels]
        if missing:
            raise ValueError(f"{what}: {missing} were never part of a solve of this session")
        return labels

    def _overlap_labels(self, labels, what):
        """the labels of an overlap query (`_device_labels`: there is no host route)"""
        return self._device_labels(labels, what, "run_overlap_search", "belief overlaps")

    def findOverlaps(self, labels=None, dims=None, number=abi.OVERLAP_TOPK, minCoeff=abi.OVERLAP_MIN_COEFF, reach=abi.OVERLAP_REACH):
        """Which of the variables' current beliefs overlap (overlap.py) -> Overlaps, the loop-closure candidates in `.pairs()`.
        labels: default every variable the last solve worked on; dims, number, minCoeff, reach as in `overlap.findOverlaps`.
        Served by ONE `run_overlap_search` where the beliefs lie (`_query_resident`): no belief travels and `stats` does not move."""
        from . import overlap
        labels = self._overlap_labels(labels, "findOverlaps")
        overlap.check_search_options(number, minCoeff, reach, self._be.N)
        if not labels:
            return overlap.findOverlaps(self.fg, [], dims, number, minCoeff, reach)
        res = self._query_resident(labels, "run_overlap_search",
                                   lambda here, place: (*overlap.search_columns(self.fg, here, dims, place), number, minCoeff, reach),
                                   lambda res, i, v: res, None)
        return overlap.Overlaps(labels, *res[labels[0]])

    def overlapVariables(self, pairs, dims=None):
        """The overlaps of pairs of variables' current beliefs (overlap.py) -> {(label_a, label_b): Overlap}, served by ONE
        `run_overlap` where the beliefs lie (`_query_resident`)."""
        from . import overlap
        pairs = [tuple(p) for p in pairs]
        labels = []
        for p in pairs:
            labels += [v for v in p if v not in labels]
        labels = self._overlap_labels(labels, "overlapVariables")
        if not pairs:
            return {}
        res = self._query_resident(labels, "run_overlap", lambda here, place: overlap.pair_columns(self.fg, pairs, dims, place),
                                   lambda res, i, v: res, None)
        return {p: overlap.overlap_from_rec(r) for p, r in zip(pairs, res[labels[0]])}

    def credibleRegions(self, labels=None, mass=(0.5, 0.9, 0.95), probs=(0.025, 0.25, 0.5, 0.75, 0.975), dims=None):
        """The credible regions of the variables' current beliefs (credible.py) -> {label: CredibleRegion}.  labels: default every
        variable the last solve worked on; mass, probs, dims as in `credible.credibleRegionAll`.  Served by ONE `run_credible`
        where the beliefs lie (`_query_resident`): no belief travels and `stats` does not move.  There is no host route."""
        from . import credible
        labels = self._device_labels(labels, "credibleRegions", "run_credible", "credible regions")
        mass, probs = credible._options(mass, probs)
        if not labels:
            return {}
        var = self.fg.getVariable
        return self._query_resident(labels, "run_credible",
                                    lambda here, place: (*credible.region_columns(self.fg, here, dims, place), mass, probs),
                                    lambda res, i, v: credible.region_from_records(var(v).varType.manifold, mass, probs, res[0][i],
                                                                                   res[1][i], res[2][i]), None)

    def credibility(self, points, dims=None):
        """The credibility of reference points under the variables' current beliefs (credible.py): points = {label: point or
        points} -> {label: Credibility(mass, logdens, n_above)}; `credible.coverage` of the result is the calibration table.
        Served by ONE `run_credible` where the beliefs lie (`_query_resident`)."""
        from . import credible
        labels = self._device_labels(list(points), "credibility", "run_credible", "credible regions")
        if not labels:
            return {}
        var = self.fg.getVariable
        packed = {v: credible.query_points(var(v).varType.manifold, dims, points[v]) for v in labels}
        return self._query_resident(labels, "run_credible",
                                    lambda here, place: (*credible.region_columns(self.fg, here, dims, place), (), (),
                                                         [packed[v][0] for v in here], False, False),
                                    lambda res, i, v: credible.credibility_from_records(res[3][res[4][i]:res[4][i + 1]], packed[v][1]),
                                    None)

    def fitBeliefMixtures(self, labels=None, maxComponents=abi.MIX_MAX, bwScale=abi.MODES_BW_SCALE, tol=abi.MIX_TOL, maxIter=abi.MIX_MAX_ITER):
        """The variables' current beliefs as Gaussian mixtures (mixture.py) -> {label: BeliefMixture}.  labels: default every
        variable the last solve worked on; maxComponents, bwScale, tol, maxIter as in `mixture.fitBeliefMixture`.  Served by ONE
        `run_modes` and ONE `run_mixture` where libnbp holds the beliefs (`_query_resident`): no belief travels and `stats` does
        not move; on the host copy, `mixture.fitBeliefMixture`."""
        from . import mixture
        K, mode_kw, kw = mixture._options(maxComponents, bwScale, tol, maxIter)
        var = self.fg.getVariable

        def run(here, place):
            return ([place[v] for v in here], [var(v).varType.manifold for v in here], [len(var(v).val) for v in here], K, mode_kw, kw)
        return self._query_resident(labels, "run_mixture", run, lambda res, i, v: res[i],
                                    lambda v, **k: mixture.fitBeliefMixture(self.fg, v, maxComponents, bwScale, tol, maxIter, **k),
                                    call=lambda be, *a: mixture.resident_mixtures(be, *a))

    def sceneGrid(self, labels=None, dims=(1, 2), n=512, extent=None, margin=abi.SCENE_MARGIN, reach=abi.SCENE_REACH, weights=None,
                  owner=False):
        """The variables' current beliefs on ONE grid (scene.py) -> Scene.  labels: a list, a regular expression, or None for every
        variable the last solve worked on whose manifold has the coordinates; the other arguments as in `scene.sceneGrid`.  Served
        by ONE `run_scene_grid` where the beliefs lie (`_query_resident`): no belief travels and `stats` does not move.  Without a
        context, on a backend without that entry point, or with a variable that has no slot in the session's context:
        `scene.sceneGrid` on the host copy (with backend=self.backend where there is a context)."""
        from . import scene
        if self._closed:
            raise RuntimeError("this SolveSession is closed")
        if labels is None and self._labels:
            per = dims if isinstance(dims, dict) else None
            need = (lambda v: max(np.atleast_1d(per[v]))) if per is not None else (lambda v: max(np.atleast_1d(dims)))
            labels = [v for v in sorted(self._labels, key=scene._natural)  # (natural order: `scene.sceneGrid`'s, so the same sums)
                      if (per is None or v in per) and self.fg.getVariable(v).varType.dim >= need(v)]
        labels, dims_of = scene.scene_labels(self.fg, labels, dims)
        args = (dims_of, n, extent, margin, reach, weights, owner)
        if self._be is None or getattr(self._be, "run_scene_grid", None) is None:
            return scene.sceneGrid(self.fg, labels, *args)
        if not labels or any(v not in self._labels for v in labels):
            return scene.sceneGrid(self.fg, labels, *args, backend=self.backend)

        def run(here, place):
            slots, mans, dd, w = scene.scene_columns(self.fg, here, dims_of, weights, place)
            nn = scene._sizes(n, len(dd[0]))
            return slots, mans, dd, nn, None if extent is None else np.asarray(extent, dtype=np.float64).reshape(-1), margin, reach, w, owner
        res = self._query_resident(labels, "run_scene_grid", run, lambda res, i, v: res, None)[labels[0]]
        return scene.scene_from_result(labels, n, res[:4], res[4])

    # ---- one solve ---------------------------------------------------------------------------------------------------------
    def solve(self, seed=0, eliminationOrder=None, ordering="qr", return_timing=False):
        """solveTree(fg, oldtree=ses.tree, ...) in the session's context -> tree (or (tree, timing) with return_timing: the
        keys of solveTree's, plus upload_s and readback_s)"""
        if self._closed:
            raise RuntimeError("this SolveSession is closed")
        whole, sp = self.fg, self.fg.solverParams
        _refuse_joint_recycling(sp, self.tree)
        if sp.isfixedlag:  # SolverAPI.jl:383-386
            from .factorgraph import fifoFreeze
            fifoFreeze(whole)
        self.stats["last"] = {"uploads": 0, "readbacks": 0, "resyncs": 0}
        T = dict.fromkeys(("init_s", "tree_s", "compile_s", "upload_s", "solve_s", "readback_s"), 0.0)
        clock = time.perf_counter
        pending = []  # initialised by this solve's init program, belief not on the host yet
        try:
            # -- plans first, on the host: the context is sized for both programs before either runs ------------------
            t = clock()
            plan, islot, n_init, istages = initStages(whole, seed) if sp.graphinit else ([], {}, 0, [])
            init_dens = _density_slots(whole)
            for sym, _, _ in plan:
                whole.getVariable(sym).initialized = True
                pending.append(sym)
            T["init_s"] += clock() - t
            t = clock()
            fg = _initialised_subgraph(whole)
            if fg is not whole and eliminationOrder is not None:
                eliminationOrder = [v for v in eliminationOrder if v in fg.variables]
            tree = bayestree.buildTreeReset(fg, eliminationOrder, ordering)
            T["tree_s"] += clock() - t
            t = clock()
            use_native = _runs_on_libnbp(self.backend)
            if use_native:
                from . import native_host
                ng = native_host.NativeGraph.from_fg(fg)
                tp = ng.build_tree(tree.eliminationOrder)
                old = getattr(self.tree, "_native", None)
                if old is not None and old._t and tp.same_ids(old):
                    tp.recycle(old, sp.incremental)
                else:
                    bayestree.setCliqueRecycling(fg, tree, self.tree, sp.incremental)
                    tp.push_statuses(tree)
                tp.pull_statuses(tree)
                tp.plan_slots(False)
                ng.place_densities(fg, tp.density_slot0())
            else:
                bayestree.setCliqueRecycling(fg, tree, self.tree, sp.incremental)
                tp = TreeProgram(fg, tree, seed=seed)
            tree_dens = _density_slots(fg)
            untouched = _untouched_variables(fg, tree)
            labels = fg.ls()
            needed = max(n_init if plan else 0, tp.n_slots)
            self.stats["slots"] = needed
            self._ensure_capacity(needed)
            if labels[:len(self._labels)] != self._labels and self._table:  # renumbered: nothing lies where it is expected
                self._resync()
            self._labels = labels
            be = self._be
            T["compile_s"] += clock() - t
            # -- graph initialisation, in this context ---------------------------------------------------------------------
            if plan:
                t = clock()
                _place_densities(whole, init_dens)
                self._upload(whole, [(v, islot[v]) for v in whole.ls()], len(whole.ls()))
                write_densities(whole, be)
                prog = None
                try:
                    prog = be.program(istages)
                    prog.run()
                    be.synchronize()
                finally:  # the program goes before its context, on the error path too
                    if prog is not None:
                        prog.close()
                for sym in pending:
                    self._table[islot[sym]] = _Resident(sym, None, None, pending=True)
                T["init_s"] += clock() - t
            # -- the tree program ------------------------------------------------------------------------------------------
            t = clock()
            _place_densities(fg, tree_dens)
            moved = [v for v in pending if tp.main[v] != islot[v]]  # (init numbers the whole graph, the tree its subgraph)
            self._readback(whole, [(v, islot[v]) for v in moved])
            pending = [v for v in pending if v not in moved]
            T["readback_s"] += clock() - t
            t = clock()
            self._upload(fg, [(v, tp.main[v]) for v in labels], len(labels))
            write_densities(fg, be)
            T["upload_s"] += clock() - t
            prog = None
            try:
                t = clock()
                prog = tp.compile(be, seed) if use_native else be.program(tp.stages, lazy_bandwidth=True)
                T["compile_s"] += clock() - t
                t = clock()
                prog.run()
                be.synchronize()
                T["solve_s"] += clock() - t
                t = clock()
                self._readback(fg, [(v, tp.main[v]) for v in labels if v not in untouched or v in pending])
                pending = []
                for v in labels:
                    fg.getVariable(v).solvedCount += 1
                if getattr(be, "run_ppe", None) is not None:
                    # setPPE! (FactorGraph.jl:200-213) of the beliefs that changed, in one launch over the resident beliefs
                    stale = [v for v in labels if fg.getVariable(v).ppe is None]
                    if stale:
                        dims = [fg.getVariable(v).varType.dim for v in stale]
                        mean, mx, idx = be.run_ppe([tp.main[v] for v in stale], [fg.getVariable(v).varType.manifold for v in stale])
                        for i, v in enumerate(stale):
                            fg.getVariable(v).ppe = MeanMaxPPE(mean[i, :dims[i]].copy(), mx[i, :dims[i]].copy(),
                                                               mean[i, :dims[i]].copy(), int(idx[i]))
                T["readback_s"] += clock() - t
            finally:
                if prog is not None:
                    prog.close()
        except BaseException:
            self._table.clear()  # the device state is unknown: the host copy wins
            for sym in pending:
                whole.getVariable(sym).initialized = False
            raise
        bayestree.setSolvedStatuses(tree, sp.downsolve)
        if use_native:
            tree._native = tp
        self.tree = tree
        self.stats["solves"] += 1
        if return_timing:
            st = tp.stats()
            st.setdefault("cliques", len(tree.cliques))
            return tree, {**T, **st}
        return tree
