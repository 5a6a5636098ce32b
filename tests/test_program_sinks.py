"""Program sinks without a GPU: the planner of include/nbp_sinks.h over the native host's stage lists.

sink_plan_check.cpp is compiled from the header alone, twice (plain, and with -fsanitize=address,undefined), and run as a
plain executable over
  * 300 random stage lists: it interprets the original and the planned order symbolically and asserts that every read sees
    the same writer in both, that a moved update lands behind its own stage and in front of its first reader, and that no
    update leaves a stage that keeps a lane-0 product of two or more densities;
  * the stage lists of three shapes, built by the native host here (config 2: the 1000-variable chain with priors every
    100 at N = 200; a 60-variable chain with priors every 10 at NBP_LANE_NARROW_MAX = 4 and at 2).
For those three the rules are restated below, over the descriptors as the native host emits them, and the planner is held
to the restatement descriptor by descriptor: which products are deferrable, which leave, and where each one goes -- plus
the counts per time step.  (What the program compiler makes of the plan -- gathered copies, seeds, fits -- needs a device:
tests/test_gpu_program_sinks.py.)"""
import os
import shutil
import subprocess
from collections import defaultdict

import pytest

from parity_utils import abi, iif

HERE = os.path.dirname(os.path.abspath(__file__))
SIDE = -2  # the side buffer (hypothesis indices, labels) as one slot

_CTYPE = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc, abi.STAGE_COPIES: abi.CopyDesc,
          abi.STAGE_DECONV: abi.ProposalDesc, abi.STAGE_COPY_POINTS: abi.CopyDesc}


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    d = tmp_path_factory.mktemp("sinks")
    plain, san = str(d / "sink_plan_check"), str(d / "sink_plan_check_san")
    src = os.path.join(HERE, "sink_plan_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O2", src, "-o", plain], check=True)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", san], check=True)
    return plain, san


def _run(checkers, *args):
    outs = []
    for exe in checkers:
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return outs[0]


def _compile(nvars, prior_every, N, narrow=None):
    """the native host's stage list and hints, on the CPU -> (stages as [(kind, [descriptors])], hints)"""
    from iif_amd import native_host
    if narrow is None:
        os.environ.pop("NBP_LANE_NARROW_MAX", None)
    else:
        os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    try:
        fg = iif.generateChainEuclid(nvars, vardims=2, priorEvery=prior_every, N=N)
        g = native_host.NativeGraph.from_fg(fg)
        nt = g.build_tree(iif.nestedDissectionOrder(fg))
        nt.plan_slots(False)
        nt.schedule(1)
        stages = []
        for kind, raw in nt.stages():
            t = _CTYPE[kind]
            n = len(raw) // abi.C.sizeof(t)
            stages.append((kind, list((t * n).from_buffer_copy(raw)) if n else []))
        hints = [[int(x != 0) for x in h] for h in nt.stage_lanes()]
        nt.close()
        g.close()
    finally:
        os.environ.pop("NBP_LANE_NARROW_MAX", None)
    return stages, hints


def _touches(kind, d):
    """what a descriptor reads and writes, the points (2 * slot) and the bandwidth (2 * slot + 1) of a slot apart
    (nbp_api.hip stage_touches)"""
    pts = lambda s: [2 * s]
    kde = lambda s: [2 * s, 2 * s + 1]
    if kind in (abi.STAGE_PROPOSALS, abi.STAGE_DECONV):
        r = [x for k in range(d.nvars) for x in pts(d.var_slot[k])]
        if d.factor_kind in (abi.F_MSGPRIOR, abi.F_PASSTHROUGH):
            r += kde(d.var_slot[1])
        if d.meas_kde > 0:
            r += kde(d.meas_kde - 1)
        w = kde(d.out_slot)
        if d.mhidx_in >= 0:
            r.append(SIDE)
        if d.mhidx_out >= 0:
            w.append(SIDE)
        return r, w
    if kind == abi.STAGE_PRODUCTS:
        r = [x for j in range(d.nfactors) for x in kde(d.in_slot[j])]
        w = kde(d.out_slot)
        if d.old_slot >= 0:  # topped up in place
            r += kde(d.old_slot)
            w += pts(d.old_slot)
        if d.labels_out >= 0:
            w.append(SIDE)
        return r, w
    if kind == abi.STAGE_COPIES:
        return kde(d.src_slot), kde(d.dst_slot)
    return pts(d.src_slot), pts(d.dst_slot)


def _up_pass(stages):
    """the stages of the up pass: between the deep copy of the clique sub graphs and the whole-slot copies of the turn"""
    copies = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_COPIES]
    return copies[0] + 1, copies[1] - 1


def _model(stages, hints):
    """-> per stage [(lane, nfactors, reads, writes)], the sink planner's kind per stage, the pass per stage"""
    first, last = _up_pass(stages)
    descs, kinds, passes = [], [], []
    for s, ((kind, ds), hint) in enumerate(zip(stages, hints)):
        lanes = hint if kind in (abi.STAGE_PROPOSALS, abi.STAGE_PRODUCTS, abi.STAGE_COPY_POINTS) else [0] * len(ds)
        descs.append([(l, d.nfactors if kind == abi.STAGE_PRODUCTS else 0, *_touches(kind, d)) for d, l in zip(ds, lanes)])
        kinds.append({abi.STAGE_PROPOSALS: 1, abi.STAGE_PRODUCTS: 2}.get(kind, 0))
        passes.append(0 if first <= s <= last else -1)
    return descs, kinds, passes


def _planner(checkers, descs, kinds, passes, path, placement=0):
    """the planner's answer through the checker -> (deferrable {(s, i)}, to {(s, i): stage}, gained {s: n}, summary)"""
    with open(path, "w") as f:
        for ds, k, ps in zip(descs, kinds, passes):
            f.write(f"S {k} {ps} {len(ds)}\n")
            for lane, nf, r, w in ds:
                f.write(" ".join(str(x) for x in [lane, nf, len(r), *r, len(w), *w]) + "\n")
    out = _run(checkers, "file", str(path), str(placement)).splitlines()
    assert out[0].startswith("ok "), out[0]
    deferrable, to, gained = set(), {}, {}
    for line in out[1:]:
        t = line.split()
        if t[0] == "def":
            deferrable.add((int(t[1]), int(t[2])))
        elif t[0] == "to":
            to[(int(t[1]), int(t[2]))] = int(t[3])
        elif t[0] == "gained":
            gained[int(t[1])] = int(t[2])
    return deferrable, to, gained, out[0]


def _restated(descs, kinds, passes):
    """The three rules, restated.  -> (deferrable {(s, i)}, to {(s, i): stage} for everything that moves, sinks (early, last))"""
    stages_of_pass = [s for s, ps in enumerate(passes) if ps == 0]
    first, last = stages_of_pass[0], stages_of_pass[-1]
    steps = [s for s in range(first + 1, last + 1) if kinds[s] == 2 and kinds[s - 1] == 1]
    # every touch of every slot in the pass, in stage order
    readers, writers = defaultdict(list), defaultdict(list)
    for s in range(first, last + 1):
        for i, (_, _, r, w) in enumerate(descs[s]):
            for x in r:
                readers[x].append((s, i))
            for x in w:
                writers[x].append((s, i))
    # -- deferrable: a lane-0 product of two or more densities with its lane-0 proposals, each feeding it alone; from the
    #    proposals' stage to the end of the pass nothing else touches what the update writes or writes what it reads
    deferrable, props_of = set(), {}
    for s in steps:
        writer_of = defaultdict(set)
        for k, (_, _, _, w) in enumerate(descs[s - 1]):
            for x in w:
                writer_of[x].add(k)
        fed = defaultdict(set)
        for i, (_, _, r, _) in enumerate(descs[s]):
            for x in r:
                for k in writer_of.get(x, ()):
                    fed[k].add(i)
        for i, (lane, nf, r, w) in enumerate(descs[s]):
            if lane != 0 or nf < 2:
                continue
            props = []
            ok = True
            for x in r:
                ks = writer_of.get(x, set())
                if not ks:
                    continue
                if len(ks) > 1:
                    ok = False
                    break
                k = next(iter(ks))
                if fed[k] != {i} or descs[s - 1][k][0] != 0:
                    ok = False
                    break
                if k not in props:
                    props.append(k)
            if not ok:
                continue
            own = {(s, i)} | {(s - 1, k) for k in props}
            written = set(w) | {x for k in props for x in descs[s - 1][k][3]}
            read = (set(r) | {x for k in props for x in descs[s - 1][k][2]}) - written
            later = lambda touch: [t for t in touch if t[0] >= s - 1 and t not in own]
            if any(later(readers[x]) or later(writers[x]) for x in written) or any(later(writers[x]) for x in read):
                continue
            deferrable.add((s, i))
            props_of[(s, i)] = props
    # -- which stages let them go: the other lane-0 products are all pass-throughs, and a later stage reads one of them
    lets_go = set()
    for s in steps:
        others = [(i, d) for i, d in enumerate(descs[s]) if d[0] == 0 and (s, i) not in deferrable]
        if others and all(d[1] == 1 for _, d in others) and any(t[0] > s for _, d in others for x in d[3] for t in readers[x]):
            lets_go.add(s)
    # -- what waits for lane 1, directly or through the chain
    hot, waits = set(), set()
    for s in range(first, last + 1):
        for i, (lane, _, r, _) in enumerate(descs[s]):
            if lane != 0 or any(x in hot for x in r):
                waits.add((s, i))
        for i, (_, _, _, w) in enumerate(descs[s]):
            for x in w:
                (hot.add if (s, i) in waits else hot.discard)(x)
    leaving = {(s, i) for (s, i) in deferrable if s in lets_go}
    leaving |= {(s - 1, k) for (s, i) in list(leaving) for k in props_of[(s, i)]}
    first_wait = next((s for s in range(first, last + 1) for i, d in enumerate(descs[s])
                       if d[0] == 0 and (s, i) in waits and (s, i) not in leaving), None)
    sink_last = steps[-1]
    sink_early = None
    if first_wait is not None:
        start = first_wait - 1 if first_wait in steps else first_wait
        sink_early = max((s for s in steps if s < start), default=None)
    to = {}
    for s in sorted(lets_go):
        target = {}
        for i in range(len(descs[s])):
            if (s, i) in deferrable:
                w = (s, i) in waits or any((s - 1, k) in waits for k in props_of[(s, i)])
                target[i] = sink_early if (sink_early is not None and sink_early >= s and not w) else sink_last
        if any(t == s for t in target.values()):
            continue  # a sink keeps what it holds itself, and then all of it
        for i, t in target.items():
            to[(s, i)] = t
            for k in props_of[(s, i)]:
                to[(s - 1, k)] = t - 1
    return deferrable, to, (sink_early, sink_last)


def _moved_per_step(stages, to):
    first, _ = _up_pass(stages)
    steps = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS and s >= first]
    return {steps.index(s): sum(1 for (ss, _) in to if ss == s) for s in {ss for (ss, _) in to} if stages[s][0] == abi.STAGE_PRODUCTS}


def _hold(checkers, stages, hints, path):
    descs, kinds, passes = _model(stages, hints)
    deferrable, to, gained, head = _planner(checkers, descs, kinds, passes, path)
    r_deferrable, r_to, sinks = _restated(descs, kinds, passes)
    assert deferrable == r_deferrable, (sorted(deferrable ^ r_deferrable)[:10], head)
    assert to == r_to, (sorted(set(to.items()) ^ set(r_to.items()))[:10], head)
    want = defaultdict(int)
    for t in to.values():
        want[t] += 1
    assert gained == dict(want)
    return descs, deferrable, to, sinks


def test_random_stage_lists(checkers):
    out = _run(checkers, "random", "300", "20261021")
    t = out.split()
    assert t[0] == "ok" and int(t[2]) == 300, out
    assert int(t[6]) > 0 and int(t[8]) > 0 and int(t[10]) > 0, out  # deferrable updates, moved ones, some to the early sink


@pytest.fixture(scope="module")
def config2():
    return _compile(1000, 100, 200)


def test_config2(checkers, config2, tmp_path):
    stages, hints = config2
    descs, deferrable, to, (early, last) = _hold(checkers, stages, hints, tmp_path / "c2.txt")
    first, _ = _up_pass(stages)
    steps = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS and s >= first]
    assert len([s for s in steps if s < _up_pass(stages)[1] + 1]) == 21
    moved = _moved_per_step(stages, to)
    assert moved == {6: 232, 7: 104, 8: 40, 9: 8, 12: 22, 13: 24, 14: 24, 15: 16, 16: 8, 17: 2, 18: 2, 19: 2}, moved
    # step 5 holds 488 deferrable products and no pass-through: they stay; the root's three stay (nothing reads the root's
    # pass-throughs: it has none)
    assert sum(1 for (s, _) in deferrable if s == steps[5]) == 488 and sum(1 for (s, _) in deferrable if s == steps[20]) == 3
    # two sinks: step 11, where lane 0 would idle until the stragglers are done, takes what steps 6-9 let go; the root's
    # step takes the rest
    assert (early, last) == (steps[11], steps[20])
    assert {t for (s, _), t in to.items() if s in steps[6:10]} == {steps[11]}
    assert {t for (s, _), t in to.items() if s in steps[12:20]} == {steps[20]}
    # from step 6 on no lane-0 product of two or more densities stays in a stage that lets its deferrable ones go
    for s in steps[6:20]:
        assert not [i for i, d in enumerate(descs[s]) if d[0] == 0 and d[1] >= 2 and (s, i) not in to], s
    # the same list with one sink: everything at the root's step
    _, to1, _, _ = _planner(checkers, *_model(stages, hints), tmp_path / "c2_last.txt", placement=1)
    assert set(to1) == set(to) and {t for (s, _), t in to1.items() if stages[s][0] == abi.STAGE_PRODUCTS} == {steps[20]}


def test_chain60_with_stragglers_in_the_up_pass(checkers, tmp_path):
    stages, hints = _compile(60, 10, 64, narrow=4)
    first, last_stage = _up_pass(stages)
    assert any(any(h) for h in hints[first:last_stage + 1])
    descs, deferrable, to, (early, last) = _hold(checkers, stages, hints, tmp_path / "c60_4.txt")
    steps = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS and s >= first]
    assert _moved_per_step(stages, to) == {6: 12, 7: 4, 12: 2, 13: 2, 14: 2, 15: 2}, _moved_per_step(stages, to)
    assert sum(1 for (s, _) in deferrable if s == steps[5]) == 28 and not [1 for (s, _) in to if s == steps[5]]
    assert early is not None and early < last and {t for (s, _), t in to.items() if s in steps[6:8]} == {early}
    assert {t for (s, _), t in to.items() if s in steps[12:16]} == {last}


def test_chain60_without_them(checkers, tmp_path):
    stages, hints = _compile(60, 10, 64, narrow=2)
    first, last_stage = _up_pass(stages)
    assert not any(any(h) for h in hints[first:last_stage + 1])
    descs, deferrable, to, (early, last) = _hold(checkers, stages, hints, tmp_path / "c60_2.txt")
    steps = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS and s >= first]
    assert early is None and {t for (s, _), t in to.items() if stages[s][0] == abi.STAGE_PRODUCTS} <= {last}
    # step 7: four deferrable products beside three lane-0 products of two densities that are not -- they stay
    assert sum(1 for (s, _) in deferrable if s == steps[7]) == 4 and not [1 for (s, _) in to if s == steps[7]]
    assert len([i for i, d in enumerate(descs[steps[7]]) if d[0] == 0 and d[1] >= 2 and (steps[7], i) not in deferrable]) == 3
