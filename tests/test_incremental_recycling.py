"""CPU: incremental solves -- fixed-lag freezing, clique recycling against an old tree, and the two schedule compilers
(solver.TreeProgram and the native host) reading the clique statuses.  Known answers: the integers the reference's
test/testBasicRecycling.jl pins.  Numeric checks run on the oracle backend at N = 100."""
import copy
import ctypes as C
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest

import incremental_cases as cases
from iif_amd import bayestree, native_host
from oracle.oracle_backend import OracleBackend
from parity_utils import iif

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {iif.abi.STAGE_PROPOSALS: iif.abi.ProposalDesc, iif.abi.STAGE_PRODUCTS: iif.abi.ProductDesc,
         iif.abi.STAGE_COPIES: iif.abi.CopyDesc, iif.abi.STAGE_COPY_POINTS: iif.abi.CopyDesc, iif.abi.STAGE_DECONV: iif.abi.ProposalDesc}
S = bayestree


def oracle(N, n_slots, side_ints=0):
    return OracleBackend(N, n_slots, side_ints, threads=8)


def symbolic_solve(fg, eliminationOrder=None, oldtree=None, compare=False):
    """what solveTree does to flags, tree and statuses, without a solve"""
    if fg.solverParams.isfixedlag:
        iif.fifoFreeze(fg)
    for v in fg.ls():
        fg.getVariable(v).initialized = True
    tree = iif.buildTreeReset(fg, eliminationOrder)
    iif.setCliqueRecycling(fg, tree, oldtree, fg.solverParams.incremental)
    native = native_twin(fg, tree, oldtree)
    for k, c in tree.cliques.items():
        assert native.clique_status(k) == (c.status, c.allmarginalized, c.isCliqReused), k
    assert native.cliques_recycled() == iif.calcCliquesRecycled(tree)
    if compare:  # both compilers on the tree as it is solved, statuses and all
        tp = iif.TreeProgram(fg, tree, seed=99, snapshot=True)
        assert native.plan_slots(True) == tp.n_slots
        assert native.main == tp.main and native.snap == tp.snap
        native.schedule(99)
        assert_same_stages(native, tp)
        native.set_owner(None, 0)  # (plan again below)
    native.plan_slots(False)
    native.schedule(0)
    bayestree.setSolvedStatuses(tree)
    for k, c in tree.cliques.items():
        assert native.clique_status(k)[0] == c.status, k
    tree._native = native
    return tree


def native_twin(fg, tree, oldtree=None):
    """the same tree in libnbp, recycled against the native twin of `oldtree` (nbp_tree_recycle)"""
    g = native_host.NativeGraph.from_fg(fg)
    nt = g.build_tree(tree.eliminationOrder)
    nt.recycle(getattr(oldtree, "_native", None), fg.solverParams.incremental)
    return nt


def assert_same_stages(nt, tp):
    got = nt.stages()
    assert len(got) == len(tp.stages)
    for s, ((kind, raw), (pk, descs)) in enumerate(zip(got, tp.stages)):
        assert kind == pk, s
        assert raw == (bytes((CTYPE[pk] * len(descs))(*descs)) if descs else b""), (s, kind, len(descs))
    st, ps = nt.stats(), tp.stats()
    for k in ("stages", "proposals", "products", "updates_up", "updates_down", "messages", "slots", "alg_bytes"):
        assert st[k] == ps[k], k


# ---- 1, 2: the graph and tree level, symbolically ---------------------------------------------------------------------
def test_fresh_tree_has_null_statuses():
    fg = cases.marginalization_graph()
    tree = iif.buildTreeReset(fg)
    assert len(tree.cliques) == 6
    assert all((c.status, c.allmarginalized, c.isCliqReused) == (S.NULL, False, False) for c in tree.cliques.values())
    assert iif.calcCliquesRecycled(tree) == (6, 0, 0, 0)


def test_basic_marginalization_known_answers():
    """calcCliquesRecycled at every point testBasicRecycling.jl asserts it, from bayestree.setCliqueRecycling and from
    nbp_tree_recycle / nbp_tree_cliques_recycled (symbolic_solve compares the two clique by clique)"""
    seen = {}

    def after(step, fg, tree, want):
        seen[step] = tree
        if want is not None:
            assert iif.calcCliquesRecycled(tree) == want, step
            assert tree._native.cliques_recycled() == want, step

    cases.marginalization_scenario(cases.marginalization_graph(), symbolic_solve, after)
    marg = lambda t: {k for k, c in t.cliques.items() if c.allmarginalized}
    t = seen[70]
    assert (t.cliques[7].frontalIDs, t.cliques[7].separatorIDs) == (["x1"], ["x2"]) and marg(t) == {7}
    assert t.cliques[7].status == S.MARGINALIZED
    t = seen[100]
    assert set(t.cliques[2].frontalIDs) == {"x8", "lm0"} and t.cliques[2].separatorIDs == ["x6"] and marg(t) == {2}
    assert (t.cliques[3].frontalIDs, set(t.cliques[3].separatorIDs)) == (["x5"], {"x4", "x6"})
    assert (t.cliques[4].frontalIDs, set(t.cliques[4].separatorIDs)) == (["x7"], {"x6", "x8"})
    t = seen[110]
    assert {k for k, c in t.cliques.items() if c.isCliqReused} == {1, 3, 4, 5, 6, 7}
    assert marg(seen[124]) == {2, 3, 4}
    assert all(c.status in (S.DOWNSOLVED, S.MARGINALIZED) for c in seen[124].cliques.values())


def test_recycling_needs_incremental_and_a_similar_downsolved_clique():
    fg, order = cases.recycle_graph()
    old = symbolic_solve(fg, order)
    iif.addFactor(fg, ["lm3"], iif.Prior(iif.Normal(3.0, 0.1)))
    tree = symbolic_solve(fg, order, oldtree=old)
    changed = tree.frontals["lm3"]  # its potentials gained the prior: not similar any more
    assert {k for k, c in tree.cliques.items() if not c.isCliqReused} == {changed}
    assert bayestree.attemptTreeSimilarClique(old, tree.cliques[changed]) is None
    other = next(k for k in tree.cliques if k != changed)
    assert bayestree.attemptTreeSimilarClique(old, tree.cliques[other]) is old.cliques[old.frontals[tree.cliques[other].frontalIDs[0]]]
    fg.solverParams.incremental = False
    assert iif.calcCliquesRecycled(symbolic_solve(fg, order, oldtree=tree)) == (len(tree.cliques), 0, 0, 0)
    fg.solverParams.incremental = True
    unsolved = iif.buildTreeReset(fg, order)  # statuses NULL: nothing to take over
    assert iif.calcCliquesRecycled(symbolic_solve(fg, order, oldtree=unsolved)) == (len(tree.cliques), 0, 0, 0)


def test_fifo_freeze_known_answers():
    fg = cases.marginalization_graph()
    assert iif.getAddHistory(fg) == ["x0", "lm0", "x1", "x2", "x3", "x4", "x5", "x6"]
    assert fg.solverParams.qfl == 2 ** 63 - 1 and not fg.solverParams.isfixedlag and fg.solverParams.incremental
    frozen = lambda: [v for v in fg.ls() if iif.isMarginalized(fg, v)]
    with pytest.warns(UserWarning, match="not initialized"):
        iif.setfreeze(fg, "x1")  # not initialised yet: left alone
    assert frozen() == []
    for v in fg.ls():
        fg.getVariable(v).initialized = True
    iif.fifoFreeze(fg)  # the default horizon reaches back for ever
    assert frozen() == []
    sp = iif.defaultFixedLagOnTree(fg, 6)
    assert (sp.isfixedlag, sp.qfl, sp.limitfixeddown) == (True, 6, True)
    iif.fifoFreeze(fg)
    assert frozen() == ["x0", "lm0"]
    cases.slide_window(fg)
    assert "x0" not in fg.ls() and not any("x0" in f for f in fg.lsf())
    assert iif.getAddHistory(fg)[:2] == ["x0", "lm0"] and iif.getAddHistory(fg)[-3:] == ["x7", "x8", "x9"]
    iif.fifoFreeze(fg)
    assert frozen() == ["lm0", "x1", "x2", "x3"]
    with pytest.warns(UserWarning, match="not initialized"):
        iif.setfreeze(fg, ["x9"])
    assert frozen() == ["lm0", "x1", "x2", "x3"]
    iif.setMarginalized(fg, "x4", True)
    assert iif.isMarginalized(fg, "x4")
    iif.unfreezeVariablesAll(fg)
    assert frozen() == [] and (sp.isfixedlag, sp.qfl, sp.limitfixeddown) == (False, 2 ** 63 - 1, False)


# ---- 3: native host against the Python mirror --------------------------------------------------------------------------
def test_recycled_scenario_trees_compile_byte_identical():
    """the trees of the reference scenario with their recycled / marginalized cliques: same slots, same stage bytes and
    statistics from both compilers, at every solve"""
    compared = []

    def solve(fg, **kw):
        tree = symbolic_solve(fg, compare=True, **kw)
        compared.append(iif.calcCliquesRecycled(tree))
        return tree

    cases.marginalization_scenario(cases.marginalization_graph(), solve, lambda *a: None)
    assert compared[-2:] == [(7, 1, 6, 0), (7, 3, 4, 0)]


@pytest.mark.parametrize("with_marginalized", [False, True])
def test_chain24_with_a_third_recycled_compiles_byte_identical(with_marginalized):
    fg = cases.chain24()
    order = iif.nestedDissectionOrder(fg)
    tree = iif.buildTreeReset(fg, order)
    g = native_host.NativeGraph.from_fg(fg)
    nt = g.build_tree(order)
    cases.mark_third_recycled(tree, nt)
    if with_marginalized:
        k = next(k for k, c in tree.cliques.items() if c.children and c.parent >= 0 and c.status == S.NULL)
        tree.cliques[k].status, tree.cliques[k].allmarginalized = S.MARGINALIZED, True
        nt.set_clique_status(k, S.MARGINALIZED)
    assert iif.calcCliquesRecycled(tree)[2] == len(tree.cliques) // 3 >= 3
    assert nt.cliques_recycled() == iif.calcCliquesRecycled(tree)
    tp = iif.TreeProgram(fg, tree, seed=5)
    full = iif.TreeProgram(fg, iif.buildTreeReset(fg, order), seed=5)
    assert nt.plan_slots(False) == tp.n_slots
    with pytest.raises(ValueError):
        nt.set_clique_status(1, S.UPRECYCLED)  # legal until the slots are planned
    nt.schedule(5)
    assert_same_stages(nt, tp)
    # 4(e): the up updates are those of the cliques that are neither recycled nor marginalized, one per step of their
    # up schedule -- from the schedules of the compile WITHOUT statuses
    live = [k for k, c in tree.cliques.items() if c.status not in (S.UPRECYCLED, S.MARGINALIZED)]
    assert tp.stats()["updates_up"] == sum(len(full.upsched[k]) for k in live) < full.stats()["updates_up"]
    assert nt.stats()["updates_up"] == tp.stats()["updates_up"]
    down_live = [k for k, c in tree.cliques.items() if c.status != S.MARGINALIZED]
    assert tp.stats()["updates_down"] == sum(len(full.dnsched[k]) for k in down_live)
    # every rank of a two-rank compile too: the stage times of a rank depend on the schedules of the whole tree
    from iif_amd.dist_solver import partition_cliques
    owner = partition_cliques(tree, 2)
    for rank in range(2):
        tpr = iif.TreeProgram(fg, tree, seed=5, owner=owner, rank=rank)
        nt.set_owner(owner, rank)
        assert nt.plan_slots(False) == tpr.n_slots
        nt.schedule(5)
        assert_same_stages(nt, tpr)
        assert nt.segments() == [tuple(x) if x[0] == "run" else (x[0], list(x[1]), list(x[2])) for x in tpr.segments], rank


def test_null_statuses_compile_as_without_the_feature():
    """a tree whose statuses are all NULL -- set explicitly, or left by a recycling pass that found nothing -- gives the
    stage bytes of a TreeProgram built from a tree nobody gave a status"""
    fg = cases.chain24()
    order = iif.nestedDissectionOrder(fg)
    tp = iif.TreeProgram(fg, iif.buildTreeReset(fg, order), seed=11, snapshot=True)
    g = native_host.NativeGraph.from_fg(fg)
    for how in ("untouched", "set", "recycle"):
        nt = g.build_tree(order)
        if how == "set":
            for k in range(1, nt.n_cliques + 1):
                nt.set_clique_status(k, S.NULL)
        elif how == "recycle":
            nt.recycle(None, True)
        assert nt.cliques_recycled() == (nt.n_cliques, 0, 0, 0)
        assert nt.plan_slots(True) == tp.n_slots
        nt.schedule(11)
        assert_same_stages(nt, tp)
    tree = iif.buildTreeReset(fg, order)
    iif.setCliqueRecycling(fg, tree, None, True)
    tq = iif.TreeProgram(fg, tree, seed=11, snapshot=True)
    assert [(k, bytes((CTYPE[k] * len(d))(*d)) if d else b"") for k, d in tq.stages] == \
           [(k, bytes((CTYPE[k] * len(d))(*d)) if d else b"") for k, d in tp.stages]


# ---- 4: on the oracle backend -------------------------------------------------------------------------------------------
def beliefs(fg):
    return {v: (fg.getVal(v).copy(), fg.getVariable(v).bw.copy()) for v in fg.ls()}


def test_all_cliques_recycled_equals_a_down_solve_only():
    """4(a): with every clique recycled no up update runs, which is what upsolve = false compiles"""
    fg = cases.chain24(n=12)
    order = iif.nestedDissectionOrder(fg)
    old = iif.solveTree(fg, eliminationOrder=order, backend=oracle, seed=3)
    assert all(c.status == S.DOWNSOLVED for c in old.cliques.values())
    a, b = copy.deepcopy(fg), copy.deepcopy(fg)
    tree, st = iif.solveTree(a, eliminationOrder=order, backend=oracle, seed=4, oldtree=old, return_timing=True)
    assert iif.calcCliquesRecycled(tree) == (len(tree.cliques), 0, len(tree.cliques), 0)
    assert st["updates_up"] == 0 and st["updates_down"] > 0
    b.solverParams.upsolve = False
    iif.solveTree(b, eliminationOrder=order, backend=oracle, seed=4)
    moved = 0
    for v in fg.ls():
        assert np.array_equal(a.getVal(v), b.getVal(v)) and np.array_equal(a.getVariable(v).bw, b.getVariable(v).bw), v
        moved += not np.array_equal(a.getVal(v), fg.getVal(v))
        assert a.getVariable(v).solvedCount == 2
    assert moved > 0


def run_marginalization_scenario(solve_backend, native=None, seed0=100):
    """the whole "basic marginalization" scenario with real solves; -> {step: beliefs after that solve}, the last graph"""
    fg = cases.marginalization_graph()
    out, count = {}, [0]

    def solve(fg, **kw):
        count[0] += 1
        return iif.solveTree(fg, backend=solve_backend, seed=seed0 + count[0], native=native, **kw)

    def after(step, fg, tree, want):
        out[step] = beliefs(fg)
        if want is not None:
            assert iif.calcCliquesRecycled(tree) == want, step
        cases.assert_ppe_band(fg, step)  # 4(d)

    cases.marginalization_scenario(fg, solve, after)
    return out, fg


@pytest.fixture(scope="module")
def marginalization_on_oracle():
    return run_marginalization_scenario(oracle)[0]


def test_basic_marginalization_on_the_oracle(marginalization_on_oracle):
    """4(b) and 4(d): the reference scenario solved -- frozen variables keep their points bit for bit, free ones move,
    the PPE band of the reference holds after every solve (asserted in run_marginalization_scenario)"""
    b = marginalization_on_oracle
    same = lambda s, t, v: np.array_equal(b[s][v][0], b[t][v][0]) and np.array_equal(b[s][v][1], b[t][v][1])
    assert same(21, 40, "x0") and same(21, 40, "lm0")       # frozen by fifoFreeze! (qfl = 6)
    assert not same(21, 40, "x1")                          # recalculated
    assert same(40, 70, "lm0") and same(40, 70, "x1")       # still frozen / now frozen too
    assert same(40, 70, "x2") and same(40, 70, "x3")
    assert same(70, 92, "lm0") and not same(70, 92, "x1")   # unfrozen, qfl = 9: lm0 only
    for v in ("x6", "x8", "lm0"):                            # clique 2, all marginalized: neither pass touches it
        assert same(92, 100, v) and same(100, 110, v)
    assert not same(100, 110, "x1")
    for v in ("x4", "x5", "x7", "x6", "x8", "lm0"):
        assert same(110, 124, v)
    assert not same(110, 124, "x1")


def test_basic_incremental_recycle_on_the_oracle():
    """4(d), second scenario: solve, add a prior on lm3, solve against the old tree; only lm3's clique is up-solved again"""
    fg, order = cases.recycle_graph()
    tree = iif.solveTree(fg, eliminationOrder=order, backend=oracle, seed=21)
    cases.assert_ppe_band(fg, "first")
    iif.addFactor(fg, ["lm3"], iif.Prior(iif.Normal(3.0, 0.1)))
    tree2, st = iif.solveTree(fg, eliminationOrder=order, backend=oracle, seed=22, oldtree=tree, return_timing=True)
    cases.assert_ppe_band(fg, "second")
    n = len(tree2.cliques)
    assert iif.calcCliquesRecycled(tree2) == (n, 0, n - 1, 0)
    full = iif.TreeProgram(fg, iif.buildTreeReset(fg, order), seed=22)
    assert st["updates_up"] == len(full.upsched[tree2.frontals["lm3"]])  # 4(e)


def test_upsolved_cliques_without_recycled_descendants_send_the_same_message():
    """4(c): at the end of the up pass a clique that was up-solved holds the separator beliefs of the full solve of the
    same graph and seed, as long as nothing below it was recycled (the random streams are keyed by clique and step)"""
    fg = cases.chain24()
    order = iif.nestedDissectionOrder(fg)
    full_tree, tree = iif.buildTreeReset(fg, order), iif.buildTreeReset(fg, order)
    root = tree.roots[0]
    recycled_top = tree.cliques[root].children[0]  # one subtree under the root is recycled whole
    stack, sub = [recycled_top], set()
    while stack:
        k = stack.pop()
        sub.add(k)
        stack += tree.cliques[k].children
    for k in sub:
        tree.cliques[k].status, tree.cliques[k].isCliqReused = S.UPRECYCLED, True
    clean = [k for k in tree.cliques if k not in sub and k != root]
    assert any(tree.cliques[k].children for k in clean) and len(sub) >= 3

    def up_pass(t):
        tp = iif.TreeProgram(fg, t, seed=17)
        be = oracle(100, tp.n_slots)
        for v in fg.ls():
            var = fg.getVariable(v)
            be.belief_write(tp.main[v], var.varType.manifold, var.val, var.bw)
        last_up = max(i for i, p in enumerate(tp.stage_pass) if p == "up") + 1
        prog = be.program(tp.stages[:last_up])
        prog.run()
        got = {(k, v): be.slot_read(tp.B[(k, v)], fg.getVariable(v).varType.manifold) for k in t.cliques for v in t.cliques[k].allIDs}
        prog.close()
        be.close()
        return got

    a, b = up_pass(full_tree), up_pass(tree)
    for k in clean:
        for v in tree.cliques[k].separatorIDs:
            assert np.array_equal(a[(k, v)][0], b[(k, v)][0]) and np.array_equal(a[(k, v)][1], b[(k, v)][1]), (k, v)
    for k in sub:  # the recycled ones still hold what they were filled with
        for v in tree.cliques[k].allIDs:
            assert np.array_equal(b[(k, v)][0], fg.getVal(v)), (k, v)
    assert any(not np.array_equal(a[(root, v)][0], b[(root, v)][0]) for v in tree.cliques[root].allIDs)


# ---- 5: two gloo ranks ---------------------------------------------------------------------------------------------------
def test_two_rank_gloo_recycled_solve_matches_single_process(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "incremental_dist_worker.py"), str(r), "2", port, outs[r]])
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    import incremental_dist_worker
    fg, tree = incremental_dist_worker.build()
    tp = iif.TreeProgram(fg, tree, seed=7)
    be = oracle(100, tp.n_slots)
    for v in fg.ls():
        var = fg.getVariable(v)
        be.slot_write(tp.main[v], var.varType.manifold, var.val, var.bw)
    be.program(tp.stages).run()
    seen = set()
    for o in outs:
        d = np.load(o)
        assert int(d["updates_up"]) + int(d["updates_down"]) > 0
        for k in d.files:
            if k.startswith("x") and not k.endswith("_bw"):
                pts, bw = be.slot_read(tp.main[k], fg.getVariable(k).varType.manifold)
                np.testing.assert_array_equal(d[k], pts)
                np.testing.assert_array_equal(d[k + "_bw"], bw)
                seen.add(k)
    assert seen == set(fg.ls())
    assert sum(int(np.load(o)["updates_up"]) for o in outs) == tp.stats()["updates_up"]


# ---- 6: joint messages ---------------------------------------------------------------------------------------------------
def test_oldtree_with_joint_messages_is_refused():
    """the joint message (differential factors) of a recycled clique has not been made to follow the reference: the
    combination raises instead of sending something else"""
    fg = cases.marginalization_graph()
    keep = ["x0", "x1", "x2"]
    for v in [v for v in fg.ls() if v not in keep]:
        iif.deleteVariable(fg, v)
    fg.solverParams.useMsgLikelihoods = True
    tree = iif.solveTree(fg, backend=oracle, seed=31)  # without an old tree the joint messages solve as ever
    cases.assert_ppe_band(fg, "joint")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="useMsgLikelihoods"):
            iif.solveTree(fg, backend=oracle, seed=32, oldtree=tree)
