"""GPU: solve sessions on libnbp (schedules compiled by the native host) against sessions on the oracle backend (the Python
mirror's schedules) with the same seeds: after every solve every belief is identical bit for bit -- SE(2) included, where both
sides keep theta resident -- and the two sessions moved the same beliefs.  On Euclid graphs the libnbp session also equals
solveTree(backend = libnbp, oldtree = ...) on a third copy."""
import numpy as np
import pytest

import incremental_cases as cases
from parity_utils import iif

pytestmark = pytest.mark.gpu


def assert_same_beliefs(a, b, what):
    assert a.ls() == b.ls()
    for v in a.ls():
        assert np.array_equal(a.getVal(v), b.getVal(v)), (what, v, np.abs(a.getVal(v) - b.getVal(v)).max())
        assert np.array_equal(a.getVariable(v).bw, b.getVariable(v).bw), (what, v)
        assert a.getVariable(v).solvedCount == b.getVariable(v).solvedCount, (what, v)


class Trio:
    """graphs edited alike: [0] a session on the oracle, [1] a session on libnbp, [2] (Euclid only) solveTree on libnbp"""

    def __init__(self, make, oracle_backend, hip_backend, seed0, third=True, reserve=0):
        self.fgs = [make() for _ in range(3 if third else 2)]
        self.ora = iif.SolveSession(self.fgs[0], backend=oracle_backend, reserve=reserve)
        self.hip = iif.SolveSession(self.fgs[1], backend=hip_backend, reserve=reserve)
        self.hip_backend, self.seed, self.tree3 = hip_backend, seed0, None

    def solve(self, **kw):
        self.seed += 1
        ta, tb = self.ora.solve(seed=self.seed, **kw), self.hip.solve(seed=self.seed, **kw)
        assert iif.calcCliquesRecycled(ta) == iif.calcCliquesRecycled(tb)
        assert [c.status for c in ta.cliques.values()] == [c.status for c in tb.cliques.values()]
        assert_same_beliefs(self.fgs[0], self.fgs[1], ("oracle session", self.seed))
        assert self.ora.stats == self.hip.stats, self.seed
        if len(self.fgs) == 3:
            self.tree3 = iif.solveTree(self.fgs[2], backend=self.hip_backend, seed=self.seed, oldtree=self.tree3, **kw)
            assert_same_beliefs(self.fgs[1], self.fgs[2], ("solveTree", self.seed))
            for v in self.fgs[1].ls():  # the estimates of the run_ppe launch over the updated beliefs, and the ones kept
                assert np.array_equal(iif.getPPESuggested(self.fgs[1], v), iif.getPPESuggested(self.fgs[2], v)), (self.seed, v)
        return ta, tb

    def close(self):
        self.ora.close()
        self.hip.close()


def test_chain24_grown_by_four_poses(oracle_backend, hip_backend):
    t = Trio(cases.chain24, oracle_backend, hip_backend, 300)
    try:
        t.solve(eliminationOrder=t.fgs[0].ls())
        old = t.hip.tree._native
        for fg in t.fgs:
            cases.grow_chain(fg, 4)
        ta, tb = t.solve(eliminationOrder=t.fgs[0].ls())
        n, marg, reused, both = iif.calcCliquesRecycled(tb)
        assert reused >= 20 and marg == 0
        assert getattr(tb, "_native", None) is not None and tb._native.same_ids(old)  # recycled by nbp_tree_recycle
        assert t.hip.stats["last"]["uploads"] == 4 and t.hip.stats["contexts"] == 1
        t.solve(eliminationOrder=t.fgs[0].ls())
        assert t.hip.stats["last"]["uploads"] == 0
    finally:
        t.close()


def test_marginalization_scenario(oracle_backend, hip_backend):
    t = Trio(cases.marginalization_graph, oracle_backend, hip_backend, 200)
    fb, frozen_before = t.fgs[1], {}
    try:
        def solve(fgs, oldtree=None, **kw):  # (the sessions and solveTree always solve against their last tree)
            frozen_before.clear()
            frozen_before.update({v: fb.getVal(v).copy() for v in fb.ls() if fb.getVariable(v).ismargin})
            return t.solve(**kw)

        def after(step, fgs, trees, want):
            for v, pts in frozen_before.items():  # what was frozen going into the solve is as it was
                if v in fb.variables and fb.getVariable(v).ismargin:
                    assert np.array_equal(fb.getVal(v), pts), (step, v)
            cases.assert_ppe_band(fb, step)

        cases.marginalization_scenario(t.fgs, solve, after)
        assert len([v for v in fb.ls() if fb.getVariable(v).ismargin]) == 6
        assert t.hip.stats["resyncs"] >= 1 and t.hip.stats["contexts"] == 1
    finally:
        t.close()


def test_context_grows(oracle_backend, hip_backend):
    t = Trio(lambda: cases.chain24(n=6), oracle_backend, hip_backend, 500)
    try:
        t.solve(eliminationOrder=t.fgs[0].ls())
        for fg in t.fgs:
            cases.grow_chain(fg, 20)
        t.solve(eliminationOrder=t.fgs[0].ls())
        assert t.hip.stats["contexts"] == 2 and t.hip.stats["resyncs"] >= 1
        assert t.hip.stats["capacity"] == t.hip.stats["slots"] + t.hip.stats["slots"] // 2
    finally:
        t.close()


def test_se2_chain_with_fixed_lag(oracle_backend, hip_backend):
    t = Trio(lambda: cases.se2_chain(12), oracle_backend, hip_backend, 400, third=False)
    fb = t.fgs[1]
    order = fb.ls()
    try:
        t.solve(eliminationOrder=order)
        written = {v: (fb.getVal(v).copy(), fb.getVariable(v).bw.copy()) for v in order}
        for fg in t.fgs:
            iif.defaultFixedLagOnTree(fg, 6)
        ta, tb = t.solve(eliminationOrder=order)
        assert [v for v in order if fb.getVariable(v).ismargin] == order[:6]
        n, marg, reused, both = iif.calcCliquesRecycled(tb)
        assert marg >= 4 and both == 0
        assert t.hip.stats["last"]["uploads"] == 0
        for v in order[:6]:  # the frozen half, bit for bit
            assert np.array_equal(fb.getVal(v), written[v][0]) and np.array_equal(fb.getVariable(v).bw, written[v][1]), v
        assert not np.array_equal(fb.getVal(order[6]), written[order[6]][0])
        cases.assert_ppe_band(fb, "se2")
    finally:
        t.close()
