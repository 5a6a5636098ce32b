"""GPU: incremental solves on libnbp, schedules compiled by the native host, against the oracle backend with the Python
mirror's schedules and the same seeds: after every solve of a growing graph every belief is identical, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import incremental_cases as cases
from parity_utils import iif

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same_beliefs(a, b, what):
    assert a.ls() == b.ls()
    for v in a.ls():
        assert np.array_equal(a.getVal(v), b.getVal(v)), (what, v, np.abs(a.getVal(v) - b.getVal(v)).max())
        assert np.array_equal(a.getVariable(v).bw, b.getVariable(v).bw), (what, v)


def both_solvers(oracle_backend, hip_backend, seed0):
    """solve(fgs, **kw): the same solveTree on the oracle (mirror) and on libnbp (native host); trees travel as pairs"""
    count = [0]

    def solve(fgs, oldtree=None, **kw):
        count[0] += 1
        old = oldtree or (None, None)
        ta = iif.solveTree(fgs[0], backend=oracle_backend, seed=seed0 + count[0], oldtree=old[0], **kw)
        tb = iif.solveTree(fgs[1], backend=hip_backend, seed=seed0 + count[0], oldtree=old[1], **kw)
        assert iif.calcCliquesRecycled(ta) == iif.calcCliquesRecycled(tb)
        assert [c.status for c in ta.cliques.values()] == [c.status for c in tb.cliques.values()]
        assert_same_beliefs(fgs[0], fgs[1], count[0])
        return ta, tb

    return solve


def test_basic_marginalization_native_host_equals_oracle_mirror(oracle_backend, hip_backend):
    solve2 = both_solvers(oracle_backend, hip_backend, 200)
    fgs = (cases.marginalization_graph(), cases.marginalization_graph())
    fb = fgs[1]
    frozen_before = {}

    def solve(fgs, **kw):
        frozen_before.clear()
        frozen_before.update({v: fb.getVal(v).copy() for v in fb.ls() if fb.getVariable(v).ismargin})
        return solve2(fgs, **kw)

    def after(step, fgs, trees, want):
        if want is not None:
            assert iif.calcCliquesRecycled(trees[1]) == want, step
        for v, pts in frozen_before.items():  # what was frozen going into the solve is read back as it was written
            assert np.array_equal(fb.getVal(v), pts), (step, v)

    cases.marginalization_scenario(fgs, solve, after)
    assert len([v for v in fb.ls() if fb.getVariable(v).ismargin]) == 6


def test_chain24_grown_by_four_poses(oracle_backend, hip_backend):
    solve = both_solvers(oracle_backend, hip_backend, 300)
    fgs = (cases.chain24(), cases.chain24())
    trees = solve(fgs, eliminationOrder=fgs[0].ls())  # natural order: the old end of the chain stays at the leaves
    for fg in fgs:
        cases.grow_chain(fg, 4)
    trees = solve(fgs, eliminationOrder=fgs[0].ls(), oldtree=trees)
    n, marg, reused, both = iif.calcCliquesRecycled(trees[1])
    assert reused >= 20 and marg == 0
    assert getattr(trees[1], "_native", None) is not None  # recycled by nbp_tree_recycle against the old native tree


def test_basic_incremental_recycle_native_host_equals_oracle_mirror(oracle_backend, hip_backend):
    """testBasicRecycling.jl:141-169: a prior on lm3 changes the potentials of one clique, every other clique is recycled"""
    solve = both_solvers(oracle_backend, hip_backend, 20)
    (fa, order), (fb, _) = cases.recycle_graph(), cases.recycle_graph()
    trees = solve((fa, fb), eliminationOrder=order)
    cases.assert_ppe_band(fb, "first")
    assert iif.calcCliquesRecycled(trees[1]) == (len(trees[1].cliques), 0, 0, 0)
    for fg in (fa, fb):
        iif.addFactor(fg, ["lm3"], iif.Prior(iif.Normal(3.0, 0.1)))
    trees = solve((fa, fb), eliminationOrder=order, oldtree=trees)
    cases.assert_ppe_band(fb, "second")
    n = len(trees[1].cliques)
    assert iif.calcCliquesRecycled(trees[1]) == (n, 0, n - 1, 0)
    changed = trees[1].frontals["lm3"]  # its potentials gained the prior: not similar any more
    assert [k for k, c in trees[1].cliques.items() if not c.isCliqReused] == [changed]
    assert [(k, c.isCliqReused) for k, c in trees[0].cliques.items()] == [(k, c.isCliqReused) for k, c in trees[1].cliques.items()]


def test_se2_chain_with_fixed_lag(oracle_backend, hip_backend):
    solve = both_solvers(oracle_backend, hip_backend, 400)
    fgs = (cases.se2_chain(12), cases.se2_chain(12))
    order = fgs[0].ls()
    trees = solve(fgs, eliminationOrder=order)
    written = {v: (fgs[1].getVal(v).copy(), fgs[1].getVariable(v).bw.copy()) for v in order[:6]}
    for fg in fgs:
        iif.defaultFixedLagOnTree(fg, 6)
    trees = solve(fgs, eliminationOrder=order, oldtree=trees)
    assert [v for v in order if fgs[1].getVariable(v).ismargin] == order[:6]
    n, marg, reused, both = iif.calcCliquesRecycled(trees[1])
    assert marg >= 4 and both == 0
    for v, (pts, bw) in written.items():  # frozen beliefs come back as they were written
        assert np.array_equal(fgs[1].getVal(v), pts) and np.array_equal(fgs[1].getVariable(v).bw, bw), v
    assert not np.array_equal(fgs[1].getVal(order[-1]), written.get(order[-1], (None,))[0])


def test_pure_c_incremental_example(tmp_path):
    """examples/solve_incremental.c: grow, freeze and solve again against the old tree from plain C"""
    csrc = os.path.join(ROOT, "incrementalinference.jl_amd", "csrc")
    exe = str(tmp_path / "solve_incremental")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "solve_incremental.c"),
                           "-o", exe, "-L", csrc, "-lnbp", f"-Wl,-rpath,{csrc}", "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reused" in out.stdout
