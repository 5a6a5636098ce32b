"""-m gpu: program lanes (nbp_api.hip plan_lanes / plan_parts / run_lanes; the hint of nbp_tree_schedule).  The cliques whose
schedules are longer than their siblings' run their rounds on a second stream, in launches of their own size, beside the
chip-filling stages of the others.  No particle and no bandwidth may depend on that: the same tree program with lanes and
with NBP_NO_LANES=1, every variable compared bit for bit -- on the first run (plain launches), the second (captured) and
the third (replayed), after new seeds on the captured program, under per-kernel timing (which runs the stages whole), for
a range that ends inside a lane-1 region (likewise) and with two-stream rounds switched on as well.

NBP_LANE_NARROW_MAX=2 makes the stages of a 60-variable chain "wide": its two-frontal end cliques are stragglers of the down
pass as they are in a 1000-variable chain at the default of 32.  Its up pass has no step of two updates, so one more case
runs at 4, where the up pass has stragglers too (the prior cliques and their neighbours)."""
import os

import numpy as np
import pytest

from parity_utils import abi, iif

pytestmark = pytest.mark.gpu

ENV_KEYS = ("NBP_NO_LANES", "NBP_LANE_NARROW_MAX", "NBP_PIPELINE_MIN")


@pytest.fixture(autouse=True)
def clean_env():
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)


def _solve(N, lanes, pipe_min=None, timing=False, split=False, narrow=2):
    """-> (posteriors after each run, diag, lane plan, stage hints).  Runs: three with the compiled seeds, one more after
    set_seeds; split: every run as two ranges, cut inside the first lane-1 region."""
    from iif_amd import native_host
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    if not lanes:
        os.environ["NBP_NO_LANES"] = "1"
    if pipe_min is not None:
        os.environ["NBP_PIPELINE_MIN"] = str(pipe_min)
    fg = iif.generateChainEuclid(60, vardims=2, priorEvery=10, N=N)
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
    hints = nt.stage_lanes()
    side = [s for s, h in enumerate(hints) if any(h)]
    cut = next(s for s in side if s - 1 in side)  # stages cut - 1 and cut both hold lane-1 descriptors
    if timing:
        be.timing_enable(True)
    be.diag(reset=True)
    outs = []

    def run():
        if split:
            prog.run(0, cut)
            prog.run(cut, -1)
        else:
            prog.run()
        be.synchronize()
        outs.append({v: be.slot_read(nt.main[v], fg.getVariable(v).varType.manifold) for v in fg.ls()})

    for _ in range(3):
        run()
    prog.set_seeds([(0x9E3779B97F4A7C15 * (i + 1)) & (2**64 - 1) for i in range(prog.num_seeds())])
    run()
    dg = be.diag()
    plan = prog.lane_plan()
    order = prog.seed_order()  # the seed map: a permutation of the caller's order, the identity unless descriptors moved
    assert sorted(order) == list(range(prog.num_seeds()))
    assert (order != list(range(len(order)))) == bool(plan), "descriptors move exactly where the program has lanes"
    prog.close()
    be.close()
    nt.close()
    g.close()
    return outs, dg, plan, hints


_REF = {}


def _ref(N, pipe_min=None, split=False, narrow=2):
    key = (N, pipe_min, split, narrow)
    if key not in _REF:
        _REF[key] = _solve(N, False, pipe_min, split=split, narrow=narrow)
    return _REF[key]


def _same(ref, got, what):
    assert len(ref) == len(got)
    for k, (a, b) in enumerate(zip(ref, got)):
        for v in a:
            np.testing.assert_array_equal(a[v][0], b[v][0], err_msg=f"{what}: run {k + 1}, points of {v}")
            np.testing.assert_array_equal(a[v][1], b[v][1], err_msg=f"{what}: run {k + 1}, bandwidth of {v}")


@pytest.mark.parametrize("N", [64, 200])
def test_lanes_change_nothing(N):
    ref, dg0, plan0, hints = _ref(N)
    got, dg1, plan1, _ = _solve(N, True)
    # the schedule marked the end cliques, and the program really ran them on lane 1
    assert sum(any(h) for h in hints) >= 4, [sum(h) for h in hints]
    assert plan0 == [] and dg0["lane_side_launches"] == 0 and dg0["lane_waits"] == 0 and dg0["lane_side_updates"] == 0, dg0
    assert any(p["lane"] == 1 for p in plan1) and any(p["wait"] >= 0 for p in plan1)
    assert dg1["lane_side_launches"] > 0 and dg1["lane_side_updates"] > 0 and dg1["lane_waits"] > 0, dg1
    for k, p in enumerate(plan1):  # a wait points backwards, at a part of the other lane that records an event
        if p["wait"] >= 0:
            assert p["wait"] < k and plan1[p["wait"]]["lane"] != p["lane"] and plan1[p["wait"]]["signals"] == 1, (k, p)
    _same(ref, got, "lanes")  # runs 1 (plain), 2 (capture), 3 (replay), 4 (new seeds on the captured program)


@pytest.mark.parametrize("N", [64, 200])
def test_lanes_under_timing_run_the_stages_whole(N):
    got, dg, _, _ = _solve(N, True, timing=True)
    assert dg["lane_side_launches"] == 0, dg
    _same(_ref(N)[0], got, "timing")


@pytest.mark.parametrize("N", [64, 200])
def test_range_that_ends_inside_a_lane_region(N):
    got, _, _, _ = _solve(N, True, split=True)
    _same(_ref(N, split=True)[0], got, "split range")
    _same(_ref(N)[0], got, "split range against whole runs")


@pytest.mark.parametrize("N", [64, 200])
def test_lanes_with_two_stream_rounds(N):
    got, dg, _, _ = _solve(N, True, pipe_min=8)
    assert dg["lane_side_launches"] > 0, dg
    _same(_ref(N, pipe_min=8)[0], got, "lanes + two-stream rounds")


def test_lanes_in_the_up_pass_too():
    """at 2 only the end cliques of the down pass are stragglers in this chain; at 4 the up pass has some as well (the prior
    cliques, whose parents read their messages from the other lane, fits and all)"""
    ref, _, _, hints = _ref(64, narrow=4)
    assert any(any(h) for h in hints[:30]) and any(any(h) for h in hints[30:]), [sum(h) for h in hints]
    got, dg, plan, _ = _solve(64, True, narrow=4)
    assert dg["lane_side_launches"] > 0 and any(p["lane"] == 1 and p["stage"] < 30 for p in plan), dg
    _same(ref, got, "lanes in both passes")
