"""-m gpu: chain promotion in the down pass (nbp_tree_schedule; DESIGN.md 3, "Lanes").  The ancestors of a down-pass
straggler run on lane 1 with it, so the chain depends on lane 0 once, where it starts.  No particle and no bandwidth may
depend on that: the same tree program with NBP_NO_LANES=1 (one lane), with NBP_LANE_NO_PROMOTE=1 (the stragglers alone) and
with the default, every variable compared bit for bit on the first run (plain launches), the second (captured), the third
(replayed) and after new seeds on the captured program.  With promotion lane 1 holds more updates, and in the lane plan the
chain's parts behind its first one wait for no lane-0 part.

The chains of tests/test_program_lane_chains.py at N = 64; NBP_LANE_NARROW_MAX = 2 .. 4 makes every step from the root's
wide, so the end cliques' chains are promoted up to the root.  One case with a prior on the frontal of the far end clique
(a longer schedule at the chain's end) and one with useMsgLikelihoods (differential factors written on lane 0 in the up pass
and read on lane 1; in these chains every ancestor of an end clique is then a straggler already, so that case holds the
results with the switch in both positions and has no promoted clique)."""
import os

import numpy as np
import pytest

from parity_utils import abi, iif

pytestmark = pytest.mark.gpu

ENV_KEYS = ("NBP_NO_LANES", "NBP_LANE_NARROW_MAX", "NBP_LANE_NO_PROMOTE")
N = 64


@pytest.fixture(autouse=True)
def clean_env():
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)


def _graph(nvars, variant):
    fg = iif.generateChainEuclid(nvars, vardims=2, priorEvery=10, N=N)
    if variant == "end_prior":
        iif.addFactor(fg, [f"x{nvars - 1}"], iif.Prior(iif.MvNormal(np.full(2, float(nvars - 1)), 0.1)))
    if variant == "msg_likelihoods":
        fg.solverParams.useMsgLikelihoods = True
    return fg


def _solve(nvars, narrow, variant, mode):
    """mode: "one_lane", "stragglers", "chains" -> (posteriors after each of four runs, diag, lane plan, stage kinds)"""
    from iif_amd import native_host
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    if mode == "one_lane":
        os.environ["NBP_NO_LANES"] = "1"
    if mode == "stragglers":
        os.environ["NBP_LANE_NO_PROMOTE"] = "1"
    fg = _graph(nvars, variant)
    g = native_host.NativeGraph.from_fg(fg)
    nt = g.build_tree(g.order_nested_dissection())
    n_slots = nt.plan_slots(True)
    need, _ = g.init_plan(0)
    be = iif.HipBackend(N, max(n_slots, need))
    ip = g.init_compile(be)
    ip.run()
    be.synchronize()
    ip.close()
    be.run_copies([abi.CopyDesc(nt.main[v], nt.snap[v]) for v in fg.ls()])
    prog = nt.compile(be, 1)
    kinds = [k for k, _ in nt.stages()]
    marked = sum(sum(h) for h in nt.stage_lanes()) + sum(sum(h) for h in nt.stage_promoted())  # (stragglers + promoted ancestors)
    be.diag(reset=True)
    outs = []

    def run():
        prog.run()
        be.synchronize()
        outs.append({v: be.slot_read(nt.main[v], fg.getVariable(v).varType.manifold) for v in fg.ls()})

    for _ in range(3):  # plain, captured, replayed
        run()
    prog.set_seeds([(0x9E3779B97F4A7C15 * (i + 1)) & (2**64 - 1) for i in range(prog.num_seeds())])
    run()
    dg = be.diag()
    plan = prog.lane_plan()
    prog.close()
    be.close()
    nt.close()
    g.close()
    return outs, dg, plan, (kinds, marked)


def _same(ref, got, what):
    assert len(ref) == len(got) == 4
    for k, (a, b) in enumerate(zip(ref, got)):
        for v in a:
            assert np.array_equal(a[v][0], b[v][0]), f"{what}: run {k + 1}, points of {v}"
            assert np.array_equal(a[v][1], b[v][1]), f"{what}: run {k + 1}, bandwidth of {v}"


def _down_side_parts(plan, kinds):
    mid = [s for s, k in enumerate(kinds) if k == abi.STAGE_COPIES][2]  # (0: the snapshot, 1: the deep copy of the clique sub graphs)
    return [p for p in plan if p["lane"] == 1 and p["stage"] > mid]


@pytest.mark.parametrize("nvars,narrow,variant", [(60, 2, "plain"), (60, 4, "plain"), (120, 2, "plain"), (100, 3, "plain"),
                                                  (60, 2, "end_prior"), (60, 2, "msg_likelihoods")])
def test_promoted_chains_change_nothing(nvars, narrow, variant):
    ref, dg0, plan0, _ = _solve(nvars, narrow, variant, "one_lane")
    strag, dg1, plan1, (kinds, marked1) = _solve(nvars, narrow, variant, "stragglers")
    chain, dg2, plan2, (_, marked2) = _solve(nvars, narrow, variant, "chains")
    assert plan0 == [] and dg0["lane_side_updates"] == 0, dg0
    _same(ref, strag, "stragglers alone against one lane")
    _same(ref, chain, "promoted chains against one lane")
    # lane 1 really ran, and ran more with the ancestors on it
    if variant == "msg_likelihoods":
        # (with the differential factors in the cliques every clique on the way to an end clique has a long schedule and is a
        #  straggler itself, at any threshold: nothing is left to promote, and the case holds the results only)
        assert marked1 == marked2 and 0 < dg1["lane_side_updates"] == dg2["lane_side_updates"], (dg1, dg2)
    else:
        assert marked1 < marked2 and 0 < dg1["lane_side_updates"] < dg2["lane_side_updates"], (marked1, marked2, dg1, dg2)
        assert len(_down_side_parts(plan1, kinds)) < len(_down_side_parts(plan2, kinds))
    for k, p in enumerate(plan2):  # a wait points backwards, at a part of the other lane that records an event
        if p["wait"] >= 0:
            assert p["wait"] < k and plan2[p["wait"]]["lane"] != p["lane"] and plan2[p["wait"]]["signals"] == 1, (k, p)
    if variant == "plain":
        # the chain forks off lane 0 once: its first part of the down pass waits (for the root's slots), no later one does
        side = _down_side_parts(plan2, kinds)
        assert side[0]["wait"] >= 0, side[0]
        assert [p for p in side[1:] if p["wait"] >= 0] == [], "a part of the promoted chain waits for lane 0"
