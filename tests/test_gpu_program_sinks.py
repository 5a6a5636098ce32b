"""-m gpu: program sinks (nbp_api.hip plan_sinks / gather_sinks; the planner of include/nbp_sinks.h).  The products of the up
pass that only the down pass reads leave the stages of their rounds and run in one or two later stages of the pass, from
gathered copies of their descriptors.  No particle and no bandwidth may depend on that: the same tree program with
NBP_NO_SINKS=1 and without, every variable compared bit for bit -- on the first run (plain launches), the second (captured)
and two replays, after nbp_program_reseed on the captured program, after set_seeds with new seeds and with the compiled
ones again, under per-kernel timing (which runs the stages whole) and for a range cut inside a region that updates moved
across (likewise).

Shapes, all at N = 64: the 60-variable chain with priors every 10 at NBP_LANE_NARROW_MAX = 4 (three stragglers in the up
pass: both sinks) and at 2 (none: one sink), a 40-variable chain at 2, and a 40-variable chain with useMsgLikelihoods
(differential factors in the cliques), held for its results only."""
import os

import numpy as np
import pytest

from parity_utils import abi, iif

pytestmark = pytest.mark.gpu

N = 64
ENV_KEYS = ("NBP_NO_SINKS", "NBP_NO_LANES", "NBP_LANE_NARROW_MAX", "NBP_SINK_PLACEMENT")
SHAPES = {"chain60_narrow4": (60, 4, False), "chain60_narrow2": (60, 2, False), "chain40_narrow2": (40, 2, False),
          "chain40_msg_likelihoods": (40, 2, True)}


@pytest.fixture(autouse=True)
def clean_env():
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)


def _solve(shape, sinks, timing=False, cut=None):
    """-> (posteriors after each of seven runs, diag, lane plan, gained per part, stage kinds).  cut: every run as two ranges"""
    from iif_amd import native_host
    from iif_amd.backend import HipProgram
    nvars, narrow, msg_lik = SHAPES[shape]
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    if not sinks:
        os.environ["NBP_NO_SINKS"] = "1"
    fg = iif.generateChainEuclid(nvars, vardims=2, priorEvery=10, N=N)
    if msg_lik:
        fg.solverParams.useMsgLikelihoods = True
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
    ctype = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc, abi.STAGE_COPIES: abi.CopyDesc,
             abi.STAGE_DECONV: abi.ProposalDesc, abi.STAGE_COPY_POINTS: abi.CopyDesc}
    compiled = HipProgram.seeds_of([(k, list((ctype[k] * (len(raw) // abi.C.sizeof(ctype[k]))).from_buffer_copy(raw)) if raw else [])
                                    for k, raw in nt.stages()])
    assert len(compiled) == prog.num_seeds()
    if timing:
        be.timing_enable(True)
    be.diag(reset=True)
    outs = []

    def run():
        if cut is not None:
            prog.run(0, cut)
            prog.run(cut, -1)
        else:
            prog.run()
        be.synchronize()
        outs.append({v: be.slot_read(nt.main[v], fg.getVariable(v).varType.manifold) for v in fg.ls()})

    for _ in range(4):  # plain, captured, replayed twice
        run()
    prog.reseed(0x5DEECE66D)
    run()
    prog.set_seeds([(0x9E3779B97F4A7C15 * (i + 1)) & (2**64 - 1) for i in range(prog.num_seeds())])
    run()
    prog.set_seeds(compiled)  # the round trip: the seeds the program was compiled with, in the caller's order
    run()
    dg = be.diag()
    plan, gained, order = prog.lane_plan(), prog.sink_plan(), prog.seed_order()
    assert sorted(order) == list(range(prog.num_seeds()))  # a permutation of the caller's order, gathered copies or not
    assert len(gained) == len(plan)
    kinds = [k for k, _ in nt.stages()]
    prog.close()
    be.close()
    nt.close()
    g.close()
    return outs, dg, plan, gained, kinds


_CACHE = {}


def _cached(shape, sinks, cut=None):
    key = (shape, sinks, cut)
    if key not in _CACHE:
        _CACHE[key] = _solve(shape, sinks, cut=cut)
    return _CACHE[key]


def _same(ref, got, what):
    assert len(ref) == len(got) == 7
    for k, (a, b) in enumerate(zip(ref, got)):
        for v in a:
            assert np.array_equal(a[v][0], b[v][0]), f"{what}: run {k + 1}, points of {v}"
            assert np.array_equal(a[v][1], b[v][1]), f"{what}: run {k + 1}, bandwidth of {v}"


def _sink_parts(plan, gained, kinds):
    """the product parts that gained updates -> [(stage, gained)]"""
    for p, n in zip(plan, gained):
        assert n == 0 or (p["lane"] == 0 and p["first_desc"] == 0 and n <= p["n"]), (p, n)
    return [(p["stage"], n) for p, n in zip(plan, gained) if n > 0 and kinds[p["stage"]] == abi.STAGE_PRODUCTS]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sinks_change_nothing(shape):
    ref, dg0, plan0, gained0, _ = _cached(shape, False)
    got, dg1, plan1, gained1, kinds = _cached(shape, True)
    assert dg0["sunk_updates"] == 0 and dg0["sink_launches"] == 0 and not any(gained0), (dg0, gained0)
    sinks = _sink_parts(plan1, gained1, kinds)
    print(shape, "sinks:", sinks, "diag:", dg1["sunk_updates"], dg1["sink_launches"])
    # runs 1 (plain), 2 (capture), 3-4 (replays), 5 (reseed), 6 (new seeds), 7 (the compiled seeds again)
    _same(ref, got, "sinks")
    per_run = sum(n for _, n in sinks)
    if shape == "chain60_narrow4":
        assert len(sinks) == 2 and per_run == 12 + 4 + 2 + 2 + 2 + 2, sinks  # (tests/test_program_sinks.py: the planner's counts)
    if shape == "chain60_narrow2":
        assert len(sinks) == 1 and per_run > 0, sinks
    if per_run:
        # counted where a launch is issued, not at replay: the plain run and the capture
        assert dg1["sunk_updates"] >= 2 * per_run and dg1["sunk_updates"] % per_run == 0 and dg1["sink_launches"] > 0, dg1
    else:
        assert dg1["sunk_updates"] == 0 and dg1["sink_launches"] == 0, dg1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sinks_under_timing_run_the_stages_whole(shape):
    got, dg, _, _, _ = _solve(shape, True, timing=True)
    assert dg["sunk_updates"] == 0 and dg["sink_launches"] == 0, dg
    _same(_cached(shape, False)[0], got, "timing")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_range_cut_inside_a_moved_region(shape):
    _, _, plan, gained, kinds = _cached(shape, True)
    sinks = _sink_parts(plan, gained, kinds)
    assert sinks or shape.startswith("chain40"), shape
    # in front of the proposals of the last sink: the updates it gains have left their stages by then  (a shape in which
    # nothing moves is cut in front of the last step of its up pass all the same)
    turn = [s for s, k in enumerate(kinds) if k == abi.STAGE_COPIES][2]  # (0: the snapshot, 1: the deep copy of the clique sub graphs)
    cut = (sinks[-1][0] if sinks else turn - 1) - 1
    got, dg, _, _, _ = _solve(shape, True, cut=cut)
    _same(_cached(shape, False, cut)[0], got, "split range")
    _same(_cached(shape, False)[0], got, "split range against whole runs")
    if len(sinks) == 1:
        assert dg["sunk_updates"] == 0, dg  # both ranges ran the stages whole
