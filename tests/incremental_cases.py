"""The growing-graph scenarios of the reference's test/testBasicRecycling.jl, shared by tests/test_incremental_recycling.py
(CPU) and tests/test_gpu_incremental.py: graphs, the edits between solves, and the known answers of calcCliquesRecycled."""
import re

import numpy as np

from parity_utils import iif

# the elimination order the reference passes once x0 is gone and x7 .. x9 are there (testBasicRecycling.jl:68)
ORDER = ["x1", "x3", "x9", "x7", "x5", "lm0", "x8", "x4", "x2", "x6"]


def marginalization_graph(N=100):
    """testBasicRecycling.jl:9-18: seven poses on a line, a prior on x0, lm0 seen from x0 and x6 only"""
    fg = iif.generateGraph_LineStep(6, poseEvery=1, landmarkEvery=7, posePriorsAt=(0,), landmarkPriorsAt=(), sightDistance=7,
                                    solverParams=iif.SolverParams(N=N))
    for i in range(1, 6):
        iif.deleteFactor(fg, f"x{i}lm0f1")
    return fg


def slide_window(fg):
    """testBasicRecycling.jl:58-64: x0 leaves, x7 .. x9 arrive, lm0 is seen again from x9"""
    iif.deleteVariable(fg, "x0")
    for i in (7, 8, 9):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
    for i in (6, 7, 8):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    iif.addFactor(fg, ["lm0", "x9"], iif.LinearRelative(iif.Normal(9.0, 0.1)))


def marginalization_scenario(fg, solve, after):
    """The "basic marginalization" test set, solve by solve.  solve(fg, **kw) -> tree stands for solveTree!; after(step, fg,
    tree, want) is called behind every solve with the tuple calcCliquesRecycled must give there (None where the reference
    asserts none) -- steps are named by the line of testBasicRecycling.jl that solves."""
    def each(fn, *args):  # `fg`: one graph, or several that are edited alike (solve and after get them as given)
        for g in (fg if isinstance(fg, (list, tuple)) else [fg]):
            fn(g, *args)

    tree = solve(fg)                                                      # :21
    after(21, fg, tree, None)
    each(iif.defaultFixedLagOnTree, 6)                                    # :30
    each(iif.fifoFreeze)                                                  # :36
    tree = solve(fg)                                                      # :40
    after(40, fg, tree, (6, 0, 0, 0))
    each(slide_window)
    tree = solve(fg, eliminationOrder=ORDER)                              # :70  clique 7 = x1 | x2 is all frozen
    after(70, fg, tree, (7, 1, 0, 0))
    each(iif.unfreezeVariablesAll)
    each(iif.defaultFixedLagOnTree, 9)                                    # :90
    tree = solve(fg, eliminationOrder=ORDER)                              # :92
    after(92, fg, tree, None)
    each(iif.setfreeze, ["x6", "x8"])                                     # :98  clique 2 = x8, lm0 | x6
    tree = solve(fg, eliminationOrder=ORDER)                              # :100
    after(100, fg, tree, (7, 1, 0, 0))
    tree = solve(fg, eliminationOrder=ORDER, oldtree=tree)                # :110
    after(110, fg, tree, (7, 1, 6, 0))
    each(iif.setfreeze, ["x4", "x5", "x7"])                               # :122  cliques 2, 3, 4
    tree = solve(fg, eliminationOrder=ORDER, oldtree=tree)                # :124
    after(124, fg, tree, (7, 3, 4, 0))
    return tree


def recycle_graph(N=100):
    """testBasicRecycling.jl:141-155 ("basic incremental recycle"), and its elimination order"""
    fg = iif.generateGraph_LineStep(3, poseEvery=1, landmarkEvery=3, posePriorsAt=(), landmarkPriorsAt=(0,), sightDistance=2,
                                    solverParams=iif.SolverParams(N=N))
    return fg, ["lm3", "x0", "x3", "x1", "x2", "lm0"]


def pose_index(label):
    return int(re.search(r"(\d+)$", label).group(1))


def assert_ppe_band(fg, what=""):
    """`isapprox(sppe[1], parse(Int, string(var)[end]), atol = 0.35)` for every variable"""
    for v in fg.ls():
        s = iif.getPPESuggested(fg, v)[0]
        assert abs(s - pose_index(v)) < 0.35, (what, v, s)


def chain24(N=100, n=24):
    """the Euclid(2) chain of BASELINE configuration 2 at test size, with synthetic initialised beliefs (tests/dist_worker.py)"""
    fg = iif.generateChainEuclid(n, vardims=2, priorEvery=8, N=N)
    for v in fg.ls():
        i = int(v[1:])
        rng = np.random.default_rng(i)
        iif.setValKDE(fg, v, rng.normal(size=(N, 2)) * 0.3 + i, np.array([0.1, 0.1]))
    return fg


def grow_chain(fg, k):
    """k more poses at the end of a generateChainEuclid(vardims = 2) chain"""
    n = len(fg.ls())
    for i in range(n, n + k):
        iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
        iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.LinearRelative(iif.MvNormal([1.0, 1.0], [0.1, 0.1])))


def se2_chain(n, N=100):
    """n SE(2) poses one metre apart along x, a prior on the first"""
    fg = iif.initfg(iif.SolverParams(N=N))
    s = np.diag([0.01, 0.01, 0.0025])
    for i in range(n):
        iif.addVariable(fg, f"x{i}", iif.SpecialEuclidean2)
    iif.addFactor(fg, ["x0"], iif.ManifoldPrior(np.zeros(3), iif.MvNormal(np.zeros(3), s)))
    for i in range(n - 1):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.ManifoldFactor(iif.MvNormal([1.0, 0.0, 0.0], s)))
    return fg


def mark_third_recycled(tree, native=None):
    """every third clique UPRECYCLED, on the Python tree and on its native twin"""
    for k, c in tree.cliques.items():
        if k % 3 == 0:
            c.status, c.isCliqReused = iif.bayestree.UPRECYCLED, True
            if native is not None:
                native.set_clique_status(k, c.status)
