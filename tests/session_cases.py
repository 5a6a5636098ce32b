"""Solve-session scenarios, written once and run on two legs: tests/test_session.py (a session on the oracle backend, and
solveTree(oldtree=) on a twin graph) and tests/test_gpu_session.py (a session on the oracle, a session on libnbp, and
solveTree(backend = libnbp, oldtree=) on a third copy).  A scenario takes the session backends (factories) and the backend of
the solveTree copy (None: no such copy -- SE(2), where a session is its own definition).

Behind every solve of every session `audit_residency` looks at what the device holds: the residency table is Python shared by
both backends, so a bug in it shows alike in both sessions and no comparison between them can see it."""
import contextlib

import numpy as np
import pytest

import incremental_cases as cases
import passthrough_cases as ptc
import ppe_cases as pc
from parity_utils import abi, coords, iif

solver = iif.solver


# ---- what a solve must leave behind -------------------------------------------------------------------------------------------------
class ResidencyError(AssertionError):
    """one finding of audit_residency: `check` names the assertion, `label` the variable (None: the table as a whole)"""

    def __init__(self, check, label, *detail):
        super().__init__(f"residency audit: {check}: {label} {detail}")
        self.check, self.label = check, label


def solved_labels(fg):
    """the variables a solve works on, in slot order: main[v] is v's place among the initialised variables"""
    return [v for v in fg.ls() if fg.getVariable(v).initialized]


def untouched_by(fg, tree):
    """the variables the solve that returned `tree` did not update.  (After the solve the statuses are those of
    setSolvedStatuses; isCliqReused / allmarginalized still say which cliques went in UPRECYCLED / MARGINALIZED.)"""
    sp, out = fg.solverParams, set()
    for cl in tree.cliques.values():
        skip_up = not sp.upsolve or cl.isCliqReused or cl.allmarginalized
        skip_dn = not sp.downsolve or cl.parent < 0 or cl.allmarginalized
        for v in cl.frontalIDs:
            frozen = fg.getVariable(v).ismargin
            if (skip_up or frozen) and (skip_dn or (frozen and sp.limitfixeddown)):
                out.add(v)
    return out


def n_updated(fg, tree):
    return sum(len(cl.frontalIDs) for cl in tree.cliques.values()) - len(untouched_by(fg, tree))


def audit_residency(ses, graph_labels, before=None):
    """The contract of a session after a solve, checked on the device itself: every variable slot holds exactly the host's
    belief.  `graph_labels`: the labels the last solve worked on, in slot order.  `before`: a copy of the table taken in front
    of that solve -- what was resident then and not touched since has not travelled.  Reads the backend directly: `ses.stats`
    does not move.  Raises ResidencyError.

    Euclid(1-3) and Circular: points and bandwidth equal bit for bit.  SE(2): x, y and bandwidth bit for bit; the rotation
    entries within 1e-15 -- a slot keeps theta = atan2(sin, cos), a read returns cos / sin of it; include/nbp_math.h states
    atan2 within 1.5 ulp (|theta| <= pi: 6.7e-16) and sincos within 1 ulp of a value <= 1 (1.1e-16)."""
    fg, table, V = ses.fg, ses._table, len(graph_labels)
    stray = sorted(s for s in table if s >= V)
    if stray:
        raise ResidencyError("entry at a slot that is no variable slot", None, stray, V)
    for slot, v in enumerate(graph_labels):
        var, e = fg.getVariable(v), table.get(slot)
        if e is None:
            raise ResidencyError("no entry", v, slot)
        if e.pending:
            raise ResidencyError("entry still pending", v, slot)
        if e.label != v:
            raise ResidencyError("entry of another variable", v, slot, e.label)
        if e.val is not var.val or e.bw is not var.bw:
            raise ResidencyError("entry does not hold the host arrays", v, slot)
    be = ses._be
    slots, mans = list(range(V)), [fg.getVariable(v).varType.manifold for v in graph_labels]
    if getattr(be, "beliefs_read", None) is not None:
        got = be.beliefs_read(slots, mans)
    else:
        got = [be.belief_read(s, m) for s, m in zip(slots, mans)]
    for v, m, (pts, bw, _) in zip(graph_labels, mans, got):
        var = fg.getVariable(v)
        if len(pts) != len(var.val):
            raise ResidencyError("count", v, len(pts), len(var.val))
        host = np.asarray(var.val).reshape(len(var.val), -1)
        exact = 2 if m == abi.SE2 else host.shape[1]
        if not np.array_equal(pts[:, :exact], host[:, :exact]):
            raise ResidencyError("points", v, np.abs(pts[:, :exact] - host[:, :exact]).max())
        if not np.array_equal(bw, var.bw):
            raise ResidencyError("bandwidth", v, bw, var.bw)
        if m == abi.SE2 and np.abs(pts[:, 2:] - host[:, 2:]).max() > 1e-15:
            raise ResidencyError("rotation", v, np.abs(pts[:, 2:] - host[:, 2:]).max())
    if before is not None and ses.stats["last"]["resyncs"] == 0:
        slot_of = {v: s for s, v in enumerate(graph_labels)}
        for v in untouched_by(fg, ses.tree):
            var, b = fg.getVariable(v), before.get(slot_of[v])
            if b is not None and b.label == v and not b.pending and b.val is var.val and b.bw is var.bw and table[slot_of[v]] is not b:
                raise ResidencyError("an untouched belief travelled", v, slot_of[v])


def assert_same_graphs(a, b, what):
    assert a.ls() == b.ls()
    for v in a.ls():
        va, vb = a.getVariable(v), b.getVariable(v)
        assert (va.initialized, va.solvedCount, va.ismargin) == (vb.initialized, vb.solvedCount, vb.ismargin), (what, v)
        if not va.initialized:
            continue
        assert np.array_equal(va.val, vb.val), (what, v, np.abs(va.val - vb.val).max())
        assert np.array_equal(va.bw, vb.bw), (what, v)


def assert_same_ppe(a, b, what):
    for v in solved_labels(a):
        assert np.array_equal(iif.getPPESuggested(a, v), iif.getPPESuggested(b, v)), (what, v)


def assert_same_trees(ta, tb, what):
    assert iif.calcCliquesRecycled(ta) == iif.calcCliquesRecycled(tb), what
    assert [(k, c.status, c.isCliqReused, c.allmarginalized) for k, c in ta.cliques.items()] == \
           [(k, c.status, c.isCliqReused, c.allmarginalized) for k, c in tb.cliques.items()], what


def assert_ppe_is_of_the_host_belief(fg, what):
    """the estimate a variable carries against calcPPE of its host belief, by the criteria of tests/ppe_cases.py (as
    test_gpu_ppe.py holds a solve's estimates): the mean within 1e-13 of the numpy walk -- on the oracle, where the estimate
    is that walk, exactly --, `suggested` the mean, `max` a point of the belief whose density is within 1e-12 of the greatest"""
    for v in solved_labels(fg):
        var = fg.getVariable(v)
        m = var.varType.manifold
        e, want = iif.getPPE(fg, v), iif.calcPPE(fg, v)
        d = np.asarray(e.mean, dtype=float) - want.mean
        for k in pc.circular_coords(m):
            d[k] = pc.wrap(d[k])
        assert np.abs(d).max() <= 1e-13, (what, v, e.mean, want.mean)
        assert np.array_equal(e.suggested, e.mean), (what, v)
        if not np.all(np.isfinite(var.bw) & (var.bw > 0)):  # (a partial density alone: no bandwidth on the other coordinates)
            assert e.max_index == -1 and np.isnan(e.max).all(), (what, v, e.max_index, e.max)
            continue
        pc.check_max(m, coords(m, var.val), var.bw, np.concatenate([e.max, np.zeros(3 - len(e.max))]), e.max_index, f"{what} {v}")


class Rig:
    """graphs edited alike: one session per backend of `backends`, each on a graph of its own (`fgs`), and -- `twin` not None --
    one more copy solved by solveTree(backend = twin, oldtree = its last tree).  Every solve asserts: the residency audit of
    every session; beliefs, bandwidths, solvedCount, freezing, stats, calcCliquesRecycled and clique statuses equal between the
    sessions; the last session equal to the solveTree copy in all of these and in getPPESuggested."""

    def __init__(self, make, backends, twin=None, seed0=0, reserve=0):
        self.fgs = [make() for _ in backends]
        self.sessions = [iif.SolveSession(fg, backend=b, reserve=reserve) for fg, b in zip(self.fgs, backends)]
        self.twin, self.twin_fg, self.twin_tree = twin, (make() if twin is not None else None), None
        self.all = self.fgs + ([self.twin_fg] if twin is not None else [])
        self.seed, self.timing, self.twin_timing = seed0, None, None
        for ses in self.sessions:
            assert ses.tree is None

    @property
    def ses(self):
        return self.sessions[-1]

    @property
    def fg(self):
        return self.fgs[-1]

    def each(self, fn, *args, **kw):
        for fg in self.all:
            fn(fg, *args, **kw)

    def audit(self, before=None):
        for i, ses in enumerate(self.sessions):
            audit_residency(ses, solved_labels(ses.fg), None if before is None else before[i])

    def solve(self, seed=None, return_timing=False, **kw):
        """-> [the tree of every session ..., the tree of the solveTree copy]"""
        self.seed = self.seed + 1 if seed is None else seed
        trees, self.timing = [], []
        for ses in self.sessions:
            before = dict(ses._table)
            if return_timing:
                tree, T = ses.solve(seed=self.seed, return_timing=True, **kw)
                self.timing.append(T)
            else:
                tree = ses.solve(seed=self.seed, **kw)
            assert ses.tree is tree
            audit_residency(ses, solved_labels(ses.fg), before)
            trees.append(tree)
        a = self.sessions[0]
        for b in self.sessions[1:]:
            assert_same_trees(a.tree, b.tree, ("sessions", self.seed))
            assert_same_graphs(a.fg, b.fg, ("sessions", self.seed))
            assert a.stats == b.stats, self.seed
        if self.twin is not None:
            r = iif.solveTree(self.twin_fg, backend=self.twin, seed=self.seed, oldtree=self.twin_tree, return_timing=return_timing, **kw)
            self.twin_tree, self.twin_timing = r if return_timing else (r, None)
            assert_same_trees(self.ses.tree, self.twin_tree, ("solveTree", self.seed))
            assert_same_graphs(self.fg, self.twin_fg, ("solveTree", self.seed))
            assert_same_ppe(self.fg, self.twin_fg, ("solveTree", self.seed))
            trees.append(self.twin_tree)
        return trees

    def close(self):
        for ses in self.sessions:
            ses.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def on_libnbp(ses):
    return solver._runs_on_libnbp(ses.backend)


# ---- 1: the chain grown by four ------------------------------------------------------------------------------------------------
def chain24_grown_by_four(backends, twin):
    with Rig(cases.chain24, backends, twin, seed0=10) as rig:
        order = lambda: rig.fg.ls()
        rig.solve(eliminationOrder=order())
        old = [getattr(s.tree, "_native", None) for s in rig.sessions]
        rig.each(cases.grow_chain, 4)
        trees = rig.solve(eliminationOrder=order(), return_timing=True)
        n, marg, reused, both = iif.calcCliquesRecycled(trees[0])
        assert reused >= 20 and marg == 0
        st, su = rig.timing[-1], rig.twin_timing
        assert set(st) == set(su) | {"upload_s", "readback_s"}
        assert {k: st[k] for k in su if not k.endswith("_s")} == {k: su[k] for k in su if not k.endswith("_s")}
        for ses, o in zip(rig.sessions, old):
            if on_libnbp(ses):  # recycled by nbp_tree_recycle
                assert o is not None and getattr(ses.tree, "_native", None) is not None and ses.tree._native.same_ids(o)
            assert ses.stats["last"]["uploads"] == 4 and ses.stats["contexts"] == 1
        rig.solve(eliminationOrder=order())
        assert rig.ses.stats["last"]["uploads"] == 0


# ---- 2: the marginalization scenario of the reference ---------------------------------------------------------------------------
def marginalization_scenario(backends, twin):
    with Rig(cases.marginalization_graph, backends, twin, seed0=100) as rig:
        count, frozen_before = [0], {}

        def solve(fgs, oldtree=None, **kw):  # (the sessions and the solveTree copy always solve against their last tree)
            count[0] += 1
            frozen_before.clear()
            for i, fg in enumerate(rig.fgs):
                frozen_before[i] = {v: (fg.getVal(v).copy(), fg.getVariable(v).bw.copy()) for v in fg.ls() if fg.getVariable(v).ismargin}
            return rig.solve(**kw)

        def after(step, fgs, trees, want):
            for i, fg in enumerate(rig.fgs):
                for v, (pts, bw) in frozen_before[i].items():
                    if v in fg.variables and fg.getVariable(v).ismargin:  # what was frozen going into the solve is as it was
                        assert np.array_equal(fg.getVal(v), pts) and np.array_equal(fg.getVariable(v).bw, bw), (step, v)
                cases.assert_ppe_band(fg, step)

        cases.marginalization_scenario(rig.all, solve, after)
        for ses in rig.sessions:
            assert count[0] == 7 and ses.stats["solves"] == 7
            assert len([v for v in ses.fg.ls() if ses.fg.getVariable(v).ismargin]) == 6
            assert ses.stats["resyncs"] >= 1 and ses.stats["contexts"] == 1  # x0 was deleted on the way: the slots were renumbered


# ---- 3: traffic ----------------------------------------------------------------------------------------------------------------------
def traffic_counts(backends, twin):
    with Rig(cases.chain24, backends, twin, reserve=400) as rig:
        ses, order = rig.ses, lambda: rig.fg.ls()
        rig.solve(eliminationOrder=order())
        assert ses.stats["last"] == {"uploads": 24, "readbacks": 24, "resyncs": 0}
        assert ses.stats["capacity"] == 400 >= ses.stats["slots"]
        rig.each(cases.grow_chain, 4)
        tree = rig.solve(eliminationOrder=order())[0]
        assert ses.stats["last"]["uploads"] == 4
        assert ses.stats["last"]["readbacks"] == n_updated(rig.fg, tree) == 28  # recycled cliques skip the up pass only
        assert iif.calcCliquesRecycled(tree)[2] >= 20
        tree = rig.solve(eliminationOrder=order())[0]  # nothing changed in between
        assert ses.stats["last"]["uploads"] == 0
        assert ses.stats["last"]["readbacks"] == n_updated(rig.fg, tree)
        assert ses.stats["contexts"] == 1 and ses.stats["resyncs"] == 0
        assert ses.stats["uploads"] == 28 and ses.stats["solves"] == 3


# ---- 4: host edits ------------------------------------------------------------------------------------------------------------------
def host_edits_win(backends, twin, how):
    pts = np.random.default_rng(5).normal(size=(100, 2)) * 0.2 + 3.3
    with Rig(lambda: cases.chain24(n=12), backends, twin, reserve=300) as rig:
        rig.solve(eliminationOrder=rig.fg.ls())
        for fg in rig.all:
            if how == "setValKDE":
                iif.setValKDE(fg, "x3", pts, np.array([0.2, 0.2]))
            else:
                fg.getVal("x3")[:] = pts
            cases.grow_chain(fg, 1)
        if how == "in_place":
            for ses in rig.sessions:
                ses.invalidate("x3")
        rig.solve(eliminationOrder=rig.fg.ls())
        for ses in rig.sessions:
            assert ses.stats["last"]["uploads"] == 2  # x3 and the new x12


def in_place_edit_without_invalidate_is_not_seen(backends):
    """the documented limit of the residency table: it knows arrays by identity.  The audit does see it: the device no longer
    holds the host copy of x3 (and of x3 alone).  No solveTree copy: solveTree reads the host."""
    with Rig(lambda: cases.chain24(n=8), backends, None, reserve=200) as rig:
        order = rig.fg.ls()
        rig.solve(eliminationOrder=order)
        for fg in rig.fgs:
            fg.getVal("x3")[:] = 0.0
        for ses in rig.sessions:
            with pytest.raises(ResidencyError) as caught:
                audit_residency(ses, solved_labels(ses.fg))
            assert (caught.value.check, caught.value.label) == ("points", "x3")
        rig.solve(eliminationOrder=order)
        for ses in rig.sessions:
            assert ses.stats["last"]["uploads"] == 0
            ses.invalidate()
        rig.solve(eliminationOrder=order)
        for ses in rig.sessions:
            assert ses.stats["last"]["uploads"] == 8 and ses.stats["resyncs"] == 0


# ---- 5: growth ------------------------------------------------------------------------------------------------------------------------
def context_grows(backends, twin):
    with Rig(lambda: cases.chain24(n=6), backends, twin, reserve=0) as rig:
        ses = rig.ses
        rig.solve(eliminationOrder=rig.fg.ls())
        need0, cap0 = ses.stats["slots"], ses.stats["capacity"]
        assert cap0 == need0 + need0 // 2 and ses.stats["contexts"] == 1
        rig.each(cases.grow_chain, 20)
        rig.solve(eliminationOrder=rig.fg.ls())
        need = ses.stats["slots"]
        assert need > cap0 and ses.stats["capacity"] == need + need // 2
        assert ses.stats["contexts"] == 2 and ses.stats["resyncs"] >= 1
        assert ses.stats["last"]["uploads"] == 26  # everything again, from the host copies


# ---- 6: renumbering ----------------------------------------------------------------------------------------------------------------
def deleted_variable_renumbers_the_slots(backends, twin):
    with Rig(lambda: cases.chain24(n=12), backends, twin, reserve=300) as rig:
        rig.solve(eliminationOrder=rig.fg.ls())
        old = [getattr(s.tree, "_native", None) for s in rig.sessions]
        rig.each(iif.deleteVariable, "x0")
        r = rig.ses.stats["resyncs"]
        rig.solve(eliminationOrder=rig.fg.ls())
        for ses, o in zip(rig.sessions, old):
            assert ses.stats["resyncs"] == r + 1 and ses.stats["contexts"] == 1
            assert ses.stats["last"]["uploads"] == 11
            if on_libnbp(ses):  # the ids moved: recycled from the labels (setCliqueRecycling + push_statuses), not by nbp_tree_recycle
                assert o is not None and not ses.tree._native.same_ids(o)


def init_graph():
    fg = cases.marginalization_graph()
    iif.addVariable(fg, "y0", iif.ContinuousScalar)  # no path to a prior
    for i in (7, 8):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
        iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    iif.addVariable(fg, "y1", iif.ContinuousScalar)
    iif.addFactor(fg, ["y0", "y1"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    return fg


def graph_initialisation_runs_in_the_session_context(backends, twin):
    """a variable graph initialisation cannot reach yet is left out of the tree, so init (whole graph) and tree (subgraph)
    number the slots differently -- the beliefs init left in slots the tree numbers otherwise come back to the host between the
    two programs; when the variable becomes reachable the subgraph is renumbered"""
    with Rig(init_graph, backends, twin) as rig:
        fa = rig.fg
        rig.solve()
        assert not fa.isInitialized("y0") and not fa.isInitialized("y1") and fa.isInitialized("x8")
        labels = solved_labels(fa)
        moved = [v for v in labels if fa.ls().index(v) != labels.index(v)]
        assert "x8" in moved
        for ses in rig.sessions:
            assert ses.stats["contexts"] == 1  # init and tree in one context
            # up: the whole graph for the init program, then what moved, to where the tree numbers it; down: what moved,
            # between the two programs, then everything the tree program updated
            assert ses.stats["last"] == {"uploads": len(fa.ls()) + len(moved), "readbacks": len(moved) + len(labels), "resyncs": 0}
        for fg in rig.all:
            iif.addFactor(fg, ["y0"], iif.Prior(iif.Normal(20.0, 0.1)))
        rig.solve()
        assert fa.isInitialized("y1")
        for ses in rig.sessions:
            assert ses.stats["resyncs"] == 1 and ses.stats["contexts"] == 1


def no_up_solve_graph():
    fg = init_graph()
    fg.solverParams.upsolve = False
    return fg


def initialised_but_not_updated(backends, twin):
    """without an up solve the frontals of the root are in no schedule: what graph initialisation left in their slots is the
    belief, and it reaches the host although the tree program never wrote it"""
    with Rig(no_up_solve_graph, backends, twin) as rig:
        tree = rig.solve()[0]
        root = [v for k in tree.roots for v in tree.cliques[k].frontalIDs]
        assert root and set(root) <= untouched_by(rig.fg, tree)
        for v in root:
            assert rig.fg.isInitialized(v) and np.all(np.isfinite(rig.fg.getVal(v))), v


# ---- 7: errors ------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def failing_programs(ses, closed):
    """every program `ses` makes raises a Python RuntimeError from run(), before anything is launched: the oracle's and
    libnbp's graph-initialisation programs come from be.program, libnbp's tree program from NativeTree.compile"""
    class Failing:
        def __init__(self, prog):
            self.prog = prog

        def run(self, *a):
            raise RuntimeError("injected")

        def close(self):
            closed.append(True)
            self.prog.close()

    be = ses._be
    real = be.program
    be.program = lambda *a, **k: Failing(real(*a, **k))
    native = iif.native_host.NativeTree if on_libnbp(ses) else None
    if native is not None:
        real_compile = native.compile
        native.compile = lambda self, *a, **k: Failing(real_compile(self, *a, **k))
    try:
        yield
    finally:
        del be.program  # (the instance attribute: the class's method shows again)
        if native is not None:
            native.compile = real_compile


def failed_program_clears_the_table_and_the_context_lives_on(backends, twin):
    """the solve that fails changes nothing on the host, so the solveTree copy simply does not make it"""
    with Rig(lambda: cases.chain24(n=8), backends, twin, reserve=200) as rig:
        order = rig.fg.ls()
        rig.solve(seed=1, eliminationOrder=order)
        bes = [ses._be for ses in rig.sessions]
        for ses in rig.sessions:
            closed = []
            with failing_programs(ses, closed):
                with pytest.raises(RuntimeError, match="injected"):
                    ses.solve(seed=2, eliminationOrder=order)
            assert closed == [True]  # the program went, on the error path too
            assert ses._table == {}
        rig.solve(seed=3, eliminationOrder=order)
        for ses, be in zip(rig.sessions, bes):
            assert ses._be is be and ses.stats["contexts"] == 1
            assert ses.stats["last"]["uploads"] == 8  # the host copy won
            assert ses.stats["solves"] == 2


# ---- 8: SE(2) ----------------------------------------------------------------------------------------------------------------------
def se2_chain_with_fixed_lag(backends):
    with Rig(lambda: cases.se2_chain(12), backends, None, seed0=400) as rig:
        order = rig.fg.ls()
        rig.solve(eliminationOrder=order)
        written = [{v: (fg.getVal(v).copy(), fg.getVariable(v).bw.copy()) for v in order} for fg in rig.fgs]
        rig.each(iif.defaultFixedLagOnTree, 6)
        trees = rig.solve(eliminationOrder=order)
        for fg, ses, tree, was in zip(rig.fgs, rig.sessions, trees, written):
            assert [v for v in order if fg.getVariable(v).ismargin] == order[:6]
            # (the root clique x11, x10 is recycled: no up solve, and a root has no down solve -- four of the six free poses move)
            assert ses.stats["last"]["uploads"] == 0 and ses.stats["last"]["readbacks"] == n_updated(fg, tree) == 4
            n, marg, reused, both = iif.calcCliquesRecycled(tree)
            assert marg >= 4 and both == 0
            for v in order[:6]:  # the frozen half, bit for bit
                assert np.array_equal(fg.getVal(v), was[v][0]) and np.array_equal(fg.getVariable(v).bw, was[v][1]), v
            assert not np.array_equal(fg.getVal(order[6]), was[order[6]][0])
            cases.assert_ppe_band(fg, "se2")


# ---- Circular: the contract says bit-identical --------------------------------------------------------------------------------------
def circular_graph():
    fg = iif.initfg(iif.SolverParams(N=100))
    for i in range(6):
        iif.addVariable(fg, f"x{i}", iif.Circular)
    iif.addFactor(fg, ["x0"], iif.PriorCircular(iif.Normal(3.0, 0.1)))  # near the cut at pi: the chain wraps
    for i in range(5):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.CircularCircular(iif.Normal(1.0, 0.1)))
    return fg


def circular_chain(backends, twin):
    with Rig(circular_graph, backends, twin, seed0=49) as rig:
        for k in range(3):
            if k == 2:
                rig.each(iif.defaultFixedLagOnTree, 3)
            tree = rig.solve(eliminationOrder=rig.fg.ls())[0]
        for ses in rig.sessions:
            assert ses.stats["last"]["uploads"] == 0 and ses.stats["last"]["readbacks"] == n_updated(ses.fg, tree) < 6
        wrapped = [v for v in rig.fg.ls() if np.any(rig.fg.getVal(v) < -2.0)]
        assert wrapped, "no belief lies beyond the cut"


# ---- particle counts that are no multiple of the wave ---------------------------------------------------------------------------------
def count_edges(backends, twin, N):
    with Rig(lambda: cases.chain24(N=N, n=23), backends, twin, seed0=600 + N) as rig:
        rig.solve(eliminationOrder=rig.fg.ls())
        rig.each(cases.grow_chain, 3)
        tree = rig.solve(eliminationOrder=rig.fg.ls())[0]
        for ses in rig.sessions:
            assert ses.stats["last"]["uploads"] == 3 and ses.stats["last"]["readbacks"] == n_updated(ses.fg, tree) == 26
        assert all(rig.fg.getVal(v).shape == (N, 2) for v in rig.fg.ls())
        rig.solve(eliminationOrder=rig.fg.ls())
        assert rig.ses.stats["last"]["uploads"] == 0 and rig.ses.stats["contexts"] == 1


# ---- pass-through densities: slots of their own behind the variables' ----------------------------------------------------------------
def euclid_passthrough_graph(N=150):
    """the ring of passthrough_cases.density as the whole prior of a Euclid(2) variable"""
    fg = iif.initfg(iif.SolverParams(N=N))
    iif.addVariable(fg, "x0", iif.ContinuousEuclid(2))
    pts, bw = ptc.density()
    iif.addFactor(fg, ["x0"], iif.PartialPriorPassThrough(iif.ContinuousEuclid(2), pts, bw), label="x0f1")
    return fg


def _extend_se2(fg):
    s = np.diag([0.01, 0.01, 0.0025])
    for i in (1, 2):
        iif.addVariable(fg, f"x{i}", iif.SpecialEuclidean2)
        iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.ManifoldFactor(iif.MvNormal([1.0, 0.0, 0.0], s)))


def _extend_euclid(fg):
    for i in (1, 2):
        iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
        iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.LinearRelative(iif.MvNormal([1.0, 1.0], [0.1, 0.1])))


def passthrough_density(backends, twin, manifold):
    """a graph whose one prior is a pass-through density, grown by two poses: the density's slot lies behind the variable
    slots, so it moves when the graph grows, and the density is written again where every program expects it"""
    make, extend = {"se2": (ptc.graph_w_priors, _extend_se2), "euclid2": (euclid_passthrough_graph, _extend_euclid)}[manifold]
    with Rig(lambda: make(N=150), backends, twin, seed0=700, reserve=40) as rig:
        fnc = [fg.getFactor("x0f1").fnc for fg in rig.fgs]
        rig.solve()
        first = [f.slot for f in fnc]
        for fg in rig.fgs:
            assert_ppe_is_of_the_host_belief(fg, (manifold, 1))
        rig.each(extend)
        rig.solve()
        assert all(f.slot != s for f, s in zip(fnc, first)), (first, [f.slot for f in fnc])
        for fg in rig.fgs:
            assert_ppe_is_of_the_host_belief(fg, (manifold, 2))
        rig.each(iif.defaultFixedLagOnTree, 2)
        rig.solve()
        for fg, ses in zip(rig.fgs, rig.sessions):
            assert [v for v in fg.ls() if fg.getVariable(v).ismargin] == ["x0"]
            assert ses.stats["last"]["uploads"] == 0 and ses.stats["contexts"] == 1
            assert_ppe_is_of_the_host_belief(fg, (manifold, 3))
            assert all(np.all(np.isfinite(fg.getVal(v))) for v in fg.ls())


# ---- a mixture, a multihypo and a nullhypo factor in the window that stays free -----------------------------------------------------------
def _mixture():
    return iif.Mixture(iif.LinearRelative, (iif.Normal(1.0, 0.1), iif.Normal(2.0, 0.5)), [0.7, 0.3])


def _rel():
    return iif.LinearRelative(iif.Normal(1.0, 0.1))


def mixed_graph():
    fg = iif.initfg(iif.SolverParams(N=100))
    for i in range(8):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
    iif.addFactor(fg, ["x0"], iif.Prior(iif.Normal(0.0, 0.1)))
    for i in range(7):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], _mixture() if i == 5 else _rel(), nullhypo=0.1 if i == 6 else 0.0)
    return fg


def _grow_mixed(fg, step):
    n = len(fg.ls())
    for i in (n, n + 1):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
    if step == 1:  # x7 -> x8 plain, x8 -> x9 a mixture
        iif.addFactor(fg, [f"x{n - 1}", f"x{n}"], _rel())
        iif.addFactor(fg, [f"x{n}", f"x{n + 1}"], _mixture())
    else:          # x9 -> x10 with a null hypothesis, x11 seen from x9 or from x10
        iif.addFactor(fg, [f"x{n - 1}", f"x{n}"], _rel(), nullhypo=0.1)
        iif.addFactor(fg, [f"x{n + 1}", f"x{n - 1}", f"x{n}"], iif.LinearRelative(iif.Normal(-1.5, 0.5)), multihypo=[1.0, 0.5, 0.5])


def mixed_graph_grown_twice(backends, twin):
    """graph initialisation of the new poses in the session, then fixed lag 6: the free window x6 .. x11 holds a mixture, two
    factors with a null hypothesis and a multihypo factor, and a mixture crosses its edge"""
    with Rig(mixed_graph, backends, twin, seed0=800, reserve=100) as rig:
        rig.solve()
        rig.each(_grow_mixed, 1)
        rig.solve()
        rig.each(_grow_mixed, 2)
        rig.each(iif.defaultFixedLagOnTree, 6)
        tree = rig.solve()[0]
        for fg, ses in zip(rig.fgs, rig.sessions):
            assert [v for v in fg.ls() if fg.getVariable(v).ismargin] == [f"x{i}" for i in range(6)]
            assert ses.stats["last"]["uploads"] == 2 and ses.stats["contexts"] == 1  # x10 and x11, for graph initialisation
            assert ses.stats["last"]["readbacks"] == n_updated(fg, tree) >= 5
            assert all(np.all(np.isfinite(fg.getVal(v))) for v in fg.ls())
