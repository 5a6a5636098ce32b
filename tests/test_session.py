"""CPU: solve sessions (iif.SolveSession) on the oracle backend -- a session solve is solveTree(oldtree = the last tree) with
the beliefs resident between solves.  Every scenario runs through a session on one graph and through solveTree on a twin
with the same seeds; on Euclid and Circular graphs the two are identical bit for bit.  The traffic counts are known answers:
what is new or edited goes up, what a program updated comes down."""
import numpy as np
import pytest

import incremental_cases as cases
from oracle.oracle_backend import OracleBackend
from parity_utils import iif


def oracle(N, n_slots, side_ints=0):
    return OracleBackend(N, n_slots, side_ints, threads=8)


def assert_same_graphs(a, b, what, ppe=True):
    assert a.ls() == b.ls()
    for v in a.ls():
        va, vb = a.getVariable(v), b.getVariable(v)
        assert np.array_equal(va.val, vb.val), (what, v, np.abs(va.val - vb.val).max())
        assert np.array_equal(va.bw, vb.bw), (what, v)
        assert (va.initialized, va.solvedCount, va.ismargin) == (vb.initialized, vb.solvedCount, vb.ismargin), (what, v)
        if ppe:
            assert np.array_equal(iif.getPPESuggested(a, v), iif.getPPESuggested(b, v)), (what, v)


def assert_same_trees(ta, tb, what):
    assert iif.calcCliquesRecycled(ta) == iif.calcCliquesRecycled(tb), what
    assert [(k, c.status, c.isCliqReused, c.allmarginalized) for k, c in ta.cliques.items()] == \
           [(k, c.status, c.isCliqReused, c.allmarginalized) for k, c in tb.cliques.items()], what


class Twin:
    """the same solves on a twin graph through solveTree(oldtree = its last tree)"""

    def __init__(self, fg):
        self.fg, self.tree = fg, None

    def solve(self, **kw):
        self.tree = iif.solveTree(self.fg, backend=oracle, oldtree=self.tree, **kw)
        return self.tree


def n_updated(fg, tree):
    """the number of variables the solve that returned `tree` updated: everything outside solveTree's `untouched` set.  (After
    the solve the statuses are those of setSolvedStatuses; isCliqReused / allmarginalized still say which cliques went in
    UPRECYCLED / MARGINALIZED.)"""
    sp, n = fg.solverParams, 0
    for cl in tree.cliques.values():
        skip_up = not sp.upsolve or cl.isCliqReused or cl.allmarginalized
        skip_dn = not sp.downsolve or cl.parent < 0 or cl.allmarginalized
        for v in cl.frontalIDs:
            frozen = fg.getVariable(v).ismargin
            n += not ((skip_up or frozen) and (skip_dn or (frozen and sp.limitfixeddown)))
    return n


# ---- 1: the chain grown by four ------------------------------------------------------------------------------------------------
def test_chain24_grown_by_four_equals_solvetree():
    fa, fb = cases.chain24(), cases.chain24()
    twin = Twin(fb)
    with iif.SolveSession(fa, backend=oracle) as ses:
        assert ses.tree is None
        ta = ses.solve(seed=11, eliminationOrder=fa.ls())
        tb = twin.solve(seed=11, eliminationOrder=fb.ls())
        assert ses.tree is ta
        assert_same_trees(ta, tb, "first")
        assert_same_graphs(fa, fb, "first")
        for fg in (fa, fb):
            cases.grow_chain(fg, 4)
        ta, st = ses.solve(seed=12, eliminationOrder=fa.ls(), return_timing=True)
        tb, su = iif.solveTree(fb, backend=oracle, seed=12, eliminationOrder=fb.ls(), oldtree=twin.tree, return_timing=True)
        assert_same_trees(ta, tb, "grown")
        assert_same_graphs(fa, fb, "grown")
        assert iif.calcCliquesRecycled(ta)[2] >= 20
        assert set(st) == set(su) | {"upload_s", "readback_s"}
        assert {k: st[k] for k in su if not k.endswith("_s")} == {k: su[k] for k in su if not k.endswith("_s")}


# ---- 2: the marginalization scenario of the reference ---------------------------------------------------------------------------
def test_marginalization_scenario_equals_solvetree():
    fa, fb = cases.marginalization_graph(), cases.marginalization_graph()
    twin, count, frozen_before = Twin(fb), [0], {}
    with iif.SolveSession(fa, backend=oracle) as ses:
        def solve(fgs, oldtree=None, **kw):  # (the session and the twin always solve against their last tree)
            count[0] += 1
            frozen_before.clear()
            frozen_before.update({v: (fa.getVal(v).copy(), fa.getVariable(v).bw.copy()) for v in fa.ls() if fa.getVariable(v).ismargin})
            return ses.solve(seed=100 + count[0], **kw), twin.solve(seed=100 + count[0], **kw)

        def after(step, fgs, trees, want):
            assert_same_trees(trees[0], trees[1], step)
            assert_same_graphs(fa, fb, step)
            for v, (pts, bw) in frozen_before.items():
                if v in fa.variables and fa.getVariable(v).ismargin:  # what was frozen going into the solve is as it was
                    assert np.array_equal(fa.getVal(v), pts) and np.array_equal(fa.getVariable(v).bw, bw), (step, v)
            cases.assert_ppe_band(fa, step)

        cases.marginalization_scenario([fa, fb], solve, after)
        assert count[0] == 7 and ses.stats["solves"] == 7
        assert len([v for v in fa.ls() if fa.getVariable(v).ismargin]) == 6
        assert ses.stats["resyncs"] >= 1  # x0 was deleted on the way: the slots were renumbered


# ---- 3: traffic ----------------------------------------------------------------------------------------------------------------------
def test_traffic_counts():
    fg = cases.chain24()
    with iif.SolveSession(fg, backend=oracle, reserve=400) as ses:
        ses.solve(seed=1, eliminationOrder=fg.ls())
        assert ses.stats["last"] == {"uploads": 24, "readbacks": 24, "resyncs": 0}
        assert ses.stats["capacity"] == 400 >= ses.stats["slots"]
        cases.grow_chain(fg, 4)
        tree = ses.solve(seed=2, eliminationOrder=fg.ls())
        assert ses.stats["last"]["uploads"] == 4
        assert ses.stats["last"]["readbacks"] == n_updated(fg, tree) == 28  # recycled cliques skip the up pass only
        assert iif.calcCliquesRecycled(tree)[2] >= 20
        tree = ses.solve(seed=3, eliminationOrder=fg.ls())  # nothing changed in between
        assert ses.stats["last"]["uploads"] == 0
        assert ses.stats["last"]["readbacks"] == n_updated(fg, tree)
        assert ses.stats["contexts"] == 1 and ses.stats["resyncs"] == 0
        assert ses.stats["uploads"] == 28 and ses.stats["solves"] == 3


def test_frozen_variables_do_not_travel(monkeypatch):
    fg = cases.chain24(n=30)
    writes, reads = [], []
    real_write, real_read = OracleBackend.belief_write, OracleBackend.belief_read
    monkeypatch.setattr(OracleBackend, "belief_write", lambda self, slot, *a, **k: (writes.append(slot), real_write(self, slot, *a, **k))[1])
    monkeypatch.setattr(OracleBackend, "belief_read", lambda self, slot, *a, **k: (reads.append(slot), real_read(self, slot, *a, **k))[1])
    with iif.SolveSession(fg, backend=oracle, reserve=500) as ses:
        ses.solve(seed=1, eliminationOrder=fg.ls())
        assert sorted(writes) == list(range(30)) == sorted(reads)
        iif.defaultFixedLagOnTree(fg, 6)
        cases.grow_chain(fg, 2)
        before = {v: (fg.getVal(v), fg.getVariable(v).bw) for v in fg.ls()}
        del writes[:], reads[:]
        tree = ses.solve(seed=2, eliminationOrder=fg.ls())
        frozen = [i for i, v in enumerate(fg.ls()) if fg.getVariable(v).ismargin]
        assert frozen == list(range(26))  # all but the last six of the add history
        assert sorted(writes) == [30, 31]
        assert not set(reads) & set(frozen) and set(reads) == set(range(26, 32))
        assert ses.stats["last"] == {"uploads": 2, "readbacks": 6, "resyncs": 0}
        for i in frozen:  # not even the array objects changed
            v = fg.ls()[i]
            assert fg.getVal(v) is before[v][0] and fg.getVariable(v).bw is before[v][1]
        assert iif.calcCliquesRecycled(tree)[1] >= 20


# ---- 4: host edits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["setValKDE", "in_place"])
def test_host_edits_win(how):
    fa, fb = cases.chain24(n=12), cases.chain24(n=12)
    twin = Twin(fb)
    pts = np.random.default_rng(5).normal(size=(100, 2)) * 0.2 + 3.3
    with iif.SolveSession(fa, backend=oracle, reserve=300) as ses:
        ses.solve(seed=1, eliminationOrder=fa.ls())
        twin.solve(seed=1, eliminationOrder=fb.ls())
        for fg in (fa, fb):
            if how == "setValKDE":
                iif.setValKDE(fg, "x3", pts, np.array([0.2, 0.2]))
            else:
                fg.getVal("x3")[:] = pts
            cases.grow_chain(fg, 1)
        if how == "in_place":
            ses.invalidate("x3")
        ses.solve(seed=2, eliminationOrder=fa.ls())
        twin.solve(seed=2, eliminationOrder=fb.ls())
        assert ses.stats["last"]["uploads"] == 2  # x3 and the new x12
        assert_same_graphs(fa, fb, how)


def test_in_place_edit_without_invalidate_is_not_seen():
    """the documented limit of the residency table: it knows arrays by identity"""
    fg = cases.chain24(n=8)
    with iif.SolveSession(fg, backend=oracle, reserve=200) as ses:
        ses.solve(seed=1, eliminationOrder=fg.ls())
        fg.getVal("x3")[:] = 0.0
        ses.solve(seed=2, eliminationOrder=fg.ls())
        assert ses.stats["last"]["uploads"] == 0
        ses.invalidate()
        ses.solve(seed=3, eliminationOrder=fg.ls())
        assert ses.stats["last"]["uploads"] == 8 and ses.stats["resyncs"] == 0


# ---- 5: growth ------------------------------------------------------------------------------------------------------------------------
def test_context_grows():
    fa, fb = cases.chain24(n=6), cases.chain24(n=6)
    twin = Twin(fb)
    with iif.SolveSession(fa, backend=oracle, reserve=0) as ses:
        ses.solve(seed=1, eliminationOrder=fa.ls())
        twin.solve(seed=1, eliminationOrder=fb.ls())
        need0, cap0 = ses.stats["slots"], ses.stats["capacity"]
        assert cap0 == need0 + need0 // 2 and ses.stats["contexts"] == 1
        for fg in (fa, fb):
            cases.grow_chain(fg, 20)
        ses.solve(seed=2, eliminationOrder=fa.ls())
        twin.solve(seed=2, eliminationOrder=fb.ls())
        need = ses.stats["slots"]
        assert need > cap0 and ses.stats["capacity"] == need + need // 2
        assert ses.stats["contexts"] == 2 and ses.stats["resyncs"] >= 1
        assert ses.stats["last"]["uploads"] == 26  # everything again, from the host copies
        assert_same_graphs(fa, fb, "grown")
        assert_same_trees(ses.tree, twin.tree, "grown")


# ---- 6: renumbering ----------------------------------------------------------------------------------------------------------------
def test_deleted_variable_renumbers_the_slots():
    fa, fb = cases.chain24(n=12), cases.chain24(n=12)
    twin = Twin(fb)
    with iif.SolveSession(fa, backend=oracle, reserve=300) as ses:
        ses.solve(seed=1, eliminationOrder=fa.ls())
        twin.solve(seed=1, eliminationOrder=fb.ls())
        for fg in (fa, fb):
            iif.deleteVariable(fg, "x0")
        r = ses.stats["resyncs"]
        ses.solve(seed=2, eliminationOrder=fa.ls())
        twin.solve(seed=2, eliminationOrder=fb.ls())
        assert ses.stats["resyncs"] == r + 1 and ses.stats["contexts"] == 1
        assert ses.stats["last"]["uploads"] == 11
        assert_same_graphs(fa, fb, "deleted")
        assert_same_trees(ses.tree, twin.tree, "deleted")


def test_graph_initialisation_runs_in_the_session_context():
    """a variable graph initialisation cannot reach yet is left out of the tree, so init (whole graph) and tree (subgraph)
    number the slots differently; when it becomes reachable the subgraph is renumbered"""
    def graph():
        fg = cases.marginalization_graph()
        iif.addVariable(fg, "y0", iif.ContinuousScalar)  # no path to a prior
        for i in (7, 8):
            iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
            iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
        iif.addVariable(fg, "y1", iif.ContinuousScalar)
        iif.addFactor(fg, ["y0", "y1"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
        return fg

    fa, fb = graph(), graph()
    twin = Twin(fb)
    with iif.SolveSession(fa, backend=oracle) as ses:
        ses.solve(seed=1)
        twin.solve(seed=1)
        assert not fa.isInitialized("y0") and not fa.isInitialized("y1") and fa.isInitialized("x8")
        assert_same_graphs(fa, fb, "first", ppe=False)
        assert ses.stats["contexts"] == 1  # init and tree in one context
        for fg in (fa, fb):
            iif.addFactor(fg, ["y0"], iif.Prior(iif.Normal(20.0, 0.1)))
        ses.solve(seed=2)
        twin.solve(seed=2)
        assert fa.isInitialized("y1")
        assert_same_graphs(fa, fb, "second")
        assert_same_trees(ses.tree, twin.tree, "second")
        assert ses.stats["resyncs"] == 1


# ---- 7: errors and closing -------------------------------------------------------------------------------------------------------------
def test_joint_messages_first_solve_runs_second_raises():
    fg = cases.marginalization_graph()
    for v in [v for v in fg.ls() if v not in ("x0", "x1", "x2")]:
        iif.deleteVariable(fg, v)
    fg.solverParams.useMsgLikelihoods = True
    ses = iif.SolveSession(fg, backend=oracle)
    ses.solve(seed=31)
    cases.assert_ppe_band(fg, "joint")
    with pytest.raises(ValueError, match="useMsgLikelihoods"):
        ses.solve(seed=32)
    ses.close()
    ses.close()
    with pytest.raises(RuntimeError, match="closed"):
        ses.solve(seed=33)


def test_failed_program_clears_the_table_and_the_context_lives_on():
    fg = cases.chain24(n=8)
    closed = []

    class Failing:
        def __init__(self, prog):
            self.prog = prog

        def run(self, *a):
            raise RuntimeError("injected")

        def close(self):
            closed.append(True)
            self.prog.close()

    with iif.SolveSession(fg, backend=oracle, reserve=200) as ses:
        ses.solve(seed=1, eliminationOrder=fg.ls())
        be = ses._be
        real = be.program
        be.program = lambda *a, **k: Failing(real(*a, **k))
        with pytest.raises(RuntimeError, match="injected"):
            ses.solve(seed=2, eliminationOrder=fg.ls())
        assert closed == [True]  # the program went, on the error path too
        be.program = real
        ses.solve(seed=3, eliminationOrder=fg.ls())
        assert ses._be is be and ses.stats["contexts"] == 1
        assert ses.stats["last"]["uploads"] == 8  # the host copy won
        assert ses.stats["solves"] == 2
    with pytest.raises(TypeError):
        iif.SolveSession(fg, backend=oracle(100, 4))


# ---- 8: SE(2) ----------------------------------------------------------------------------------------------------------------------
def test_se2_chain_with_fixed_lag():
    fg = cases.se2_chain(12)
    order = fg.ls()
    with iif.SolveSession(fg, backend=oracle) as ses:
        ses.solve(seed=401, eliminationOrder=order)
        written = {v: (fg.getVal(v).copy(), fg.getVariable(v).bw.copy()) for v in order}
        iif.defaultFixedLagOnTree(fg, 6)
        tree = ses.solve(seed=402, eliminationOrder=order)
        assert [v for v in order if fg.getVariable(v).ismargin] == order[:6]
        # (the root clique x11, x10 is recycled: no up solve, and a root has no down solve -- four of the six free poses move)
        assert ses.stats["last"]["uploads"] == 0 and ses.stats["last"]["readbacks"] == n_updated(fg, tree) == 4
        n, marg, reused, both = iif.calcCliquesRecycled(tree)
        assert marg >= 4 and both == 0
        for v in order[:6]:  # the frozen half, bit for bit
            assert np.array_equal(fg.getVal(v), written[v][0]) and np.array_equal(fg.getVariable(v).bw, written[v][1]), v
        assert not np.array_equal(fg.getVal(order[6]), written[order[6]][0])
        cases.assert_ppe_band(fg, "se2")


# ---- Circular: the contract says bit-identical --------------------------------------------------------------------------------------
def test_circular_chain_equals_solvetree():
    def graph():
        fg = iif.initfg(iif.SolverParams(N=100))
        for i in range(6):
            iif.addVariable(fg, f"x{i}", iif.Circular)
        iif.addFactor(fg, ["x0"], iif.PriorCircular(iif.Normal(3.0, 0.1)))  # near the cut at pi: the chain wraps
        for i in range(5):
            iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.CircularCircular(iif.Normal(1.0, 0.1)))
        return fg

    fa, fb = graph(), graph()
    twin = Twin(fb)
    with iif.SolveSession(fa, backend=oracle) as ses:
        for k in range(3):
            if k == 2:
                for fg in (fa, fb):
                    iif.defaultFixedLagOnTree(fg, 3)
            tree = ses.solve(seed=50 + k, eliminationOrder=fa.ls())
            twin.solve(seed=50 + k, eliminationOrder=fb.ls())
            assert_same_graphs(fa, fb, k)
        assert ses.stats["last"]["uploads"] == 0 and ses.stats["last"]["readbacks"] == n_updated(fa, tree) < 6
