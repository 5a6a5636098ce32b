"""Chain promotion in the down pass without a GPU (nbp_tree_schedule; DESIGN.md 3, "Lanes"): the ancestors of a down-pass
straggler travel on lane 1 with it, from the straggler towards the root, while they have a round in a wide step.

The rule is restated here over the Python mirror's tree and schedules -- ASAP times, updates per time step, stragglers,
promoted ancestors, the cap of 64 side updates per step -- and the marks of the native host (nbp_tree_stage_lanes: the
stragglers, as before; nbp_tree_stage_promoted: their promoted ancestors; the program runs both on lane 1) are held to it
descriptor by descriptor: a product stage holds the updates of its running cliques in clique order, a points-only copy
stage the separators of the cliques that start, a proposal goes where the product that reads it goes.  NBP_LANE_NO_PROMOTE=1
must give the stragglers alone, the up pass must not depend on it, a tree whose promoted cliques would hold more than 64
updates in one step keeps the stragglers alone, the share of one rank of several marks nothing.

lane_chain_check.cpp (include/nbp_lanes.h alone, plain and with -fsanitize=address,undefined, run as a plain executable):
random stage lists with promoted chains through nbp_lane_sweep and nbp_lane_reach."""
import os
import shutil
import subprocess

import pytest

from parity_utils import abi, iif

HERE = os.path.dirname(os.path.abspath(__file__))
SIDE_MAX = 64  # the cap of nbp_tree_schedule
ROUND_UPDATES = 200  # what a round beside a wide stage costs, in updates of a wide stage (nbp_tree_schedule)
ENV_KEYS = ("NBP_LANE_NARROW_MAX", "NBP_LANE_NO_PROMOTE")
_CTYPE = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc, abi.STAGE_COPIES: abi.CopyDesc,
          abi.STAGE_DECONV: abi.ProposalDesc, abi.STAGE_COPY_POINTS: abi.CopyDesc}


@pytest.fixture(autouse=True)
def clean_env():
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)


def _native(fg, narrow, promote, world=1):
    """the native host's stage list and hints -> (stages as [(kind, [descriptors])], Marks)"""
    from iif_amd import native_host
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    if narrow is not None:
        os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    if not promote:
        os.environ["NBP_LANE_NO_PROMOTE"] = "1"
    g = native_host.NativeGraph.from_fg(fg)
    nt = g.build_tree(iif.nestedDissectionOrder(fg))
    if world > 1:
        nt.set_owner(nt.partition(world), 0)
    nt.plan_slots(False)
    nt.schedule(1)
    stages = []
    for kind, raw in nt.stages():
        t = _CTYPE[kind]
        n = len(raw) // abi.C.sizeof(t)
        stages.append((kind, list((t * n).from_buffer_copy(raw)) if n else []))
    lanes, promoted = nt.stage_lanes(), nt.stage_promoted()
    nt.close()
    g.close()
    # the stragglers' mark and the promoted ancestors' are kept apart (nbp_tree_stage_lanes / nbp_tree_stage_promoted) and
    # never both set; the compiled program runs either on lane 1: the hint it gets is their union
    assert all(not (a and b) for la, pr in zip(lanes, promoted) for a, b in zip(la, pr))
    return stages, Marks([[a | b for a, b in zip(la, pr)] for la, pr in zip(lanes, promoted)], lanes)


class Marks(list):
    """per stage the lane of every descriptor as the program gets it; .stragglers: the stragglers' mark alone"""

    def __init__(self, union, stragglers):
        super().__init__(union)
        self.stragglers = stragglers


def _times(tp, tree, down):
    """ASAP times of a pass -> (rounds, start, finish, updates per time step)"""
    rounds = tp.dnrounds if down else tp.uprounds
    start, finish = {}, {}
    if down:
        for c in sorted(tree.cliques, key=lambda c: (tp.depths[c], c)):
            par = tree.cliques[c].parent
            start[c] = finish[par] if par >= 0 else 0
            finish[c] = start[c] + len(rounds[c])
    else:
        for c in sorted(tree.cliques, key=lambda c: (tp.heights[c], c)):
            start[c] = max([finish[x] for x in tree.cliques[c].children] + [0])
            finish[c] = start[c] + len(rounds[c])
    T = max(finish.values())
    count = [sum(len(rounds[c][t - start[c]]) for c in tree.cliques if start[c] <= t < finish[c]) for t in range(T)]
    return rounds, start, finish, count


def _held(cliques, rounds, start, finish, T):
    return [sum(len(rounds[c][t - start[c]]) for c in cliques if start[c] <= t < finish[c]) for t in range(T)]


def _rule(tp, tree, down, narrow, promote):
    """the documented rule -> (stragglers, marked cliques, promoted cliques the cap threw out)"""
    rounds, start, finish, count = _times(tp, tree, down)
    steps = lambda c: range(start[c], finish[c])
    side = {c for c in tree.cliques if any(count[t] <= narrow for t in steps(c)) and any(count[t] > narrow for t in steps(c))}
    if max(_held(side, rounds, start, finish, len(count)), default=0) > SIDE_MAX:
        side = set()
    if not (down and promote):
        return side, set(side), set()
    chain = set(side)
    for c in sorted(side):
        # a straggler whose rounds, at ROUND_UPDATES each, are no more than the updates of the wide steps from its start on
        # hides beside them as it is: its chain stays where it was
        if len(rounds[c]) * ROUND_UPDATES <= sum(n for n in count[start[c]:] if n > narrow):
            continue
        a = tree.cliques[c].parent
        while a >= 0 and any(count[t] > narrow for t in steps(a)):  # the first ancestor without a round in a wide step ends the walk
            chain.add(a)
            a = tree.cliques[a].parent
    if max(_held(chain, rounds, start, finish, len(count)), default=0) > SIDE_MAX:
        return side, set(side), chain - side
    return side, chain, set()


def _expected_hints(tp, tree, stages, up_marked, down_marked):
    """per stage the hint of every descriptor that the marked cliques imply ({stage: [lane]}: update and copy-points stages)"""
    prod = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS]
    mid = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_COPIES][1]  # (0: the deep copy of the clique sub graphs)
    out = {}
    for down, marked, at in ((False, up_marked, [s for s in prod if s < mid]), (True, down_marked, [s for s in prod if s > mid])):
        rounds, start, finish, count = _times(tp, tree, down)
        at = iter(at)
        for t, n in enumerate(count):
            if not n:
                continue
            s = next(at)
            out[s] = [int(c in marked) for c in sorted(tree.cliques) if start[c] <= t < finish[c] for _ in rounds[c][t - start[c]]]
            assert len(out[s]) == len(stages[s][1]), (down, t)
            reader = {}  # a proposal goes where the product that reads it goes
            for d, h in zip(stages[s][1], out[s]):
                for j in range(d.nfactors):
                    reader[d.in_slot[j]] = h
            out[s - 1] = [reader[p.out_slot] for p in stages[s - 1][1]]
        assert next(at, None) is None
    # the points-only copies that feed a clique, per time step and per link of a chain of cliques without updates of their own
    _, start, finish, count = _times(tp, tree, True)
    copies = iter(s for s, (k, _) in enumerate(stages) if k == abi.STAGE_COPY_POINTS and s > mid)
    for t in range(len(count) + 1):
        rnd = {}
        for c in sorted((c for c in tree.cliques if start[c] == t and tree.cliques[c].parent >= 0), key=lambda c: (tp.depths[c], c)):
            rnd[c] = rnd[tree.cliques[c].parent] + 1 if tree.cliques[c].parent in rnd else 0
        for r in sorted(set(rnd.values())):
            row = [int(c in down_marked) for c in sorted(rnd) if rnd[c] == r for _ in tree.cliques[c].separatorIDs]
            if row:
                s = next(copies)
                assert len(row) == len(stages[s][1]), (t, r)
                out[s] = row
    assert next(copies, None) is None
    return out


def _case(nvars, prior_every, narrow):
    fg = iif.generateChainEuclid(nvars, vardims=2, priorEvery=prior_every, N=64)
    tree = iif.buildTreeReset(fg, iif.nestedDissectionOrder(fg))
    return fg, tree, iif.TreeProgram(fg, tree, seed=1)


def _check_hints(stages, hints, want):
    for s, (kind, descs) in enumerate(stages):
        assert len(hints[s]) == len(descs)
        assert hints[s] == want.get(s, [0] * len(descs)), (s, kind)


# chains whose end cliques are deeper than the wide part; at 2 .. 4 every step from the root's is wide and the chain is
# promoted up to the root, at 6 and 12 the top of the tree is narrow and the walk ends below it
CASES = [(40, 10, 4), (60, 10, 2), (60, 10, 4), (100, 7, 3), (120, 10, 2), (120, 10, 6), (120, 10, 12)]


@pytest.mark.parametrize("nvars,prior_every,narrow", CASES)
def test_marked_set_is_stragglers_ancestors_and_their_copies(nvars, prior_every, narrow):
    fg, tree, tp = _case(nvars, prior_every, narrow)
    uside, umarked, _ = _rule(tp, tree, False, narrow, True)
    dside, dmarked, dropped = _rule(tp, tree, True, narrow, True)
    assert dside and dmarked > dside and not dropped, (dside, dmarked)  # the case does promote something
    for c in dmarked - dside:  # (what the rule restated above must mean: an ancestor of a straggler, linked to it by marked cliques)
        assert any(tree.cliques[k].parent == c for k in dmarked)
    if narrow >= 6:
        roots = [c for c in tree.cliques if tree.cliques[c].parent < 0]
        assert not set(roots) & dmarked, "the walk ends at the first ancestor whose rounds are all narrow"
    stages, hints = _native(fg, narrow, True)
    _check_hints(stages, hints, _expected_hints(tp, tree, stages, umarked, dmarked))
    _check_hints(stages, hints.stragglers, _expected_hints(tp, tree, stages, uside, dside))  # the stragglers' own mark is what it was


@pytest.mark.parametrize("nvars,prior_every,narrow", CASES)
def test_no_promote_gives_the_stragglers_alone_and_the_up_pass_does_not_move(nvars, prior_every, narrow):
    fg, tree, tp = _case(nvars, prior_every, narrow)
    uside, umarked, _ = _rule(tp, tree, False, narrow, False)
    dside, dmarked, _ = _rule(tp, tree, True, narrow, False)
    assert dmarked == dside and umarked == uside
    stages, hints = _native(fg, narrow, False)
    _check_hints(stages, hints, _expected_hints(tp, tree, stages, umarked, dmarked))
    assert hints.stragglers == list(hints), "nothing promoted"
    stages1, hints1 = _native(fg, narrow, True)
    assert hints1.stragglers == hints.stragglers
    mid = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_COPIES][1]
    assert list(hints1[:mid]) == list(hints[:mid]), "up-pass hints"
    assert list(hints1[mid:]) != list(hints[mid:])
    # the stage list is what it was: same stages, same descriptors, same order, same seeds
    assert [(k, [bytes(d) for d in ds]) for k, ds in stages1] == [(k, [bytes(d) for d in ds]) for k, ds in stages]


def _forest(chains, nvars=60, prior_every=10):
    """that many separate 60-variable chains in one graph: every time step holds `chains` times the updates of one chain"""
    import numpy as np
    fg = iif.initfg(iif.SolverParams(N=64))
    for k in range(chains):
        for i in range(nvars):
            iif.addVariable(fg, f"c{k}x{i}", iif.ContinuousEuclid(2))
            if i % prior_every == 0:
                iif.addFactor(fg, [f"c{k}x{i}"], iif.Prior(iif.MvNormal(np.full(2, float(i)), 0.1)))
            if i > 0:
                iif.addFactor(fg, [f"c{k}x{i - 1}", f"c{k}x{i}"], iif.LinearRelative(iif.MvNormal(np.full(2, 1.0), 0.1)))
    return fg


@pytest.mark.parametrize("chains,kept", [(16, True), (17, False)])
def test_cap_counts_the_promoted_cliques(chains, kept):
    """One 60-variable chain: two end cliques are stragglers (2 updates in a step), their ancestors hold 4 updates in the
    root's steps.  At NBP_LANE_NARROW_MAX = 40, 16 chains hold 32 and 64 (the cap: kept), 17 chains 34 and 68: the promotion
    is dropped and the 34 stragglers stay marked."""
    narrow = 40
    fg = _forest(chains)
    tree = iif.buildTreeReset(fg, iif.nestedDissectionOrder(fg))
    tp = iif.TreeProgram(fg, tree, seed=1)
    rounds, start, finish, count = _times(tp, tree, True)
    dside, dmarked, dropped = _rule(tp, tree, True, narrow, True)
    assert len(dside) == 2 * chains and max(_held(dside, rounds, start, finish, len(count))) == 2 * chains
    assert max(_held(dmarked | dropped, rounds, start, finish, len(count))) == 4 * chains
    assert (dmarked > dside and not dropped) if kept else (dmarked == dside and dropped)
    stages, hints = _native(fg, narrow, True)
    _check_hints(stages, hints, _expected_hints(tp, tree, stages, _rule(tp, tree, False, narrow, True)[1], dmarked))


def test_a_straggler_that_hides_beside_the_wide_steps_keeps_its_ancestors_on_lane_0():
    """20 chains of 120: the end clique that starts one step earlier has 20 x (44 + 29) updates of wide steps beside its seven
    rounds and needs no promotion, the other has 20 x 29 beside its six and does."""
    narrow = 40
    fg = _forest(20, nvars=120)
    tree = iif.buildTreeReset(fg, iif.nestedDissectionOrder(fg))
    tp = iif.TreeProgram(fg, tree, seed=1)
    dside, dmarked, dropped = _rule(tp, tree, True, narrow, True)
    assert len(dside) == 40 and not dropped
    with_chain = {c for c in dside if tree.cliques[c].parent in dmarked}
    assert len(with_chain) == 20 and all(tree.cliques[c].parent not in dmarked for c in dside - with_chain)
    stages, hints = _native(fg, narrow, True)
    _check_hints(stages, hints, _expected_hints(tp, tree, stages, _rule(tp, tree, False, narrow, True)[1], dmarked))


def test_sweep_over_random_promoted_chains(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    src = os.path.join(HERE, "lane_chain_check.cpp")
    plain, san = str(tmp_path / "lane_chain_check"), str(tmp_path / "lane_chain_check_san")
    subprocess.run([cxx, "-std=c++17", "-O2", src, "-o", plain], check=True)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", san], check=True)
    outs = []
    for exe in (plain, san):
        r = subprocess.run([exe, "300", "20261020"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    f = outs[0].split()
    assert f[:3] == ["ok", "lists", "300"], outs[0]
    got = dict(zip(f[1::2], (int(x) for x in f[2::2])))
    assert got["lane1"] > 0 and got["promoted"] > 300 and got["waits"] > 0 and got["conflicts"] > 0, outs[0]


def test_sharded_tree_marks_nothing():
    fg, tree, tp = _case(60, 10, 2)
    assert _rule(tp, tree, True, 2, True)[1]
    _, hints = _native(fg, 2, True, world=2)
    assert not any(any(h) for h in hints)
