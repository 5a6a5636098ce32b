"""Program lanes without a GPU: the hint of the native host (nbp_tree_schedule) and the cross-lane sweep of include/nbp_lanes.h.

lane_plan_check.cpp is compiled from the header alone, twice (plain, and with -fsanitize=address,undefined), and run as a
plain executable over
  * the config-2 stage list (1000-variable Euclid(2) chain, priors every 100, N = 200), built by the native host here,
  * a 60-variable chain with priors every 10,
  * 200 random stage lists with random hints, wrong ones included.
For every pair of parts on different lanes that touch a slot, one of them writing, a happens-before path must exist; no wait
points forward; the join covers every lane-1 part (the checker says how).  Config 2 specifically: which time steps lane 0
leaves to lane 1, how many cliques lane 1 holds in each pass -- against the rule restated here over the Python mirror's tree
(the seed map of the reordered descriptors is the library's, built at nbp_program_finalize: tests/test_gpu_program_lanes.py
holds it)."""
import os
import shutil
import subprocess

import pytest

from parity_utils import abi, iif

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NARROW_MAX, SIDE_MAX = 32, 64  # the defaults of nbp_tree_schedule


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    d = tmp_path_factory.mktemp("lanes")
    plain, san = str(d / "lane_plan_check"), str(d / "lane_plan_check_san")
    src = os.path.join(HERE, "lane_plan_check.cpp")
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


def _reads_writes(kind, d):
    """what a descriptor reads and writes, slot by slot (nbp_api.hip stage_reads / stage_writes)"""
    if kind in (abi.STAGE_PROPOSALS, abi.STAGE_DECONV):
        r = [d.var_slot[k] for k in range(d.nvars)]
        if d.factor_kind in (abi.F_MSGPRIOR, abi.F_PASSTHROUGH):
            r.append(d.var_slot[1])
        if d.meas_kde > 0:
            r.append(d.meas_kde - 1)
        return r, [d.out_slot]
    if kind == abi.STAGE_PRODUCTS:
        r = [d.in_slot[j] for j in range(d.nfactors)]
        if d.old_slot >= 0:
            r.append(d.old_slot)
        return r, [d.out_slot]
    return [d.src_slot], [d.dst_slot]


_CTYPE = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc, abi.STAGE_COPIES: abi.CopyDesc,
          abi.STAGE_DECONV: abi.ProposalDesc, abi.STAGE_COPY_POINTS: abi.CopyDesc}


def _compile(nvars, prior_every, N, narrow=None):
    """the native host's stage list and hints, on the CPU -> (stages as [(kind, [descriptors])], hints, fg, order)"""
    from iif_amd import native_host
    if narrow is None:
        os.environ.pop("NBP_LANE_NARROW_MAX", None)
    else:
        os.environ["NBP_LANE_NARROW_MAX"] = str(narrow)
    try:
        fg = iif.generateChainEuclid(nvars, vardims=2, priorEvery=prior_every, N=N)
        order = iif.nestedDissectionOrder(fg)
        g = native_host.NativeGraph.from_fg(fg)
        nt = g.build_tree(order)
        nt.plan_slots(False)
        nt.schedule(1)
        stages = []
        for kind, raw in nt.stages():
            t = _CTYPE[kind]
            n = len(raw) // abi.C.sizeof(t)
            stages.append((kind, list((t * n).from_buffer_copy(raw)) if n else []))
        hints = nt.stage_lanes()
        nt.close()
        g.close()
    finally:
        os.environ.pop("NBP_LANE_NARROW_MAX", None)
    return stages, hints, fg, order


def _parts_file(stages, hints, path):
    """the parts as nbp_api.hip cuts them: per stage its lane-0 descriptors, then its lane-1 descriptors; whole-slot copies stay
    on lane 0; an empty stage is a barrier; a trailing barrier part is the join"""
    lines = []
    for s, ((kind, descs), hint) in enumerate(zip(stages, hints)):
        if not descs:
            lines.append(f"{s} 0 1 0 0")
            continue
        for lane in (0, 1):
            rs, ws = [], []
            for d, h in zip(descs, hint):
                if (h if kind in (abi.STAGE_PROPOSALS, abi.STAGE_PRODUCTS, abi.STAGE_COPY_POINTS) else 0) == lane:
                    r, w = _reads_writes(kind, d)
                    rs += r
                    ws += w
            if rs or ws:
                lines.append(" ".join(str(x) for x in [s, lane, 0, len(rs), *rs, len(ws), *ws]))
    lines.append(f"{len(stages)} 0 1 0 0")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


@pytest.fixture(scope="module")
def config2():
    return _compile(1000, 100, 200)


def test_random_stage_lists_with_random_hints(checkers):
    out = _run(checkers, "random", "200", "20261020")
    assert out.startswith("ok lists 200 "), out
    assert int(out.split()[6]) > 0 and int(out.split()[8]) > 0, out  # waits were derived, conflicts were met


def test_config2_sweep(checkers, config2, tmp_path):
    stages, hints, _, _ = config2
    _parts_file(stages, hints, tmp_path / "c2.txt")
    out = _run(checkers, "file", str(tmp_path / "c2.txt"))
    head = out.splitlines()[0].split()
    assert head[0] == "ok" and int(head[4]) > 0 and int(head[6]) > 0, out  # lane-1 parts, waits


def test_chain60_sweep(checkers, tmp_path):
    for narrow in (2, 4):
        stages, hints, _, _ = _compile(60, 10, 64, narrow=narrow)
        assert any(any(h) for h in hints), narrow
        _parts_file(stages, hints, tmp_path / f"c60_{narrow}.txt")
        out = _run(checkers, "file", str(tmp_path / f"c60_{narrow}.txt"))
        assert out.startswith("ok "), out


def _passes(stages):
    """stage indices of the update rounds (product stages) of the up pass and of the down pass: the whole-slot copy stage
    between them separates the two"""
    prod = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_PRODUCTS]
    mid = [s for s, (k, _) in enumerate(stages) if k == abi.STAGE_COPIES][1]  # (0: the deep copy of the clique sub graphs)
    return [s for s in prod if s < mid], [s for s in prod if s > mid]


def _rule(tp, tree):
    """the stragglers by the rule, restated over the Python mirror's schedules: ASAP times, updates per time step, a clique is
    a straggler of a pass when its schedule covers a narrow step and a wide one -> per pass (clique set, lane-1 updates per step)"""
    out = []
    for down in (False, True):
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
        side = {c for c in tree.cliques
                if any(count[t] <= NARROW_MAX for t in range(start[c], finish[c])) and any(count[t] > NARROW_MAX for t in range(start[c], finish[c]))}
        held = [sum(len(rounds[c][t - start[c]]) for c in side if start[c] <= t < finish[c]) for t in range(T)]
        if max(held, default=0) > SIDE_MAX:
            side, held = set(), [0] * T
        out.append((side, count, held))
    return out


def test_config2_hint(config2):
    stages, hints, fg, order = config2
    up, dn = _passes(stages)
    assert len(up) == 21 and len(dn) == 14, (len(up), len(dn))
    lane1 = lambda s: sum(hints[s])
    lane0 = lambda s: len(hints[s]) - sum(hints[s])
    # lane 0 has nothing in up steps 10-11 nor in down steps 8-12: those steps exist for the stragglers alone
    assert [lane0(up[t]) for t in (10, 11)] == [0, 0] and all(lane0(up[t]) > 0 for t in range(21) if t not in (10, 11))
    assert [lane0(dn[t]) for t in range(8, 13)] == [0] * 5 and lane0(dn[13]) == 1 and all(lane0(dn[t]) > 0 for t in range(8))
    # the proposals of a lane-1 update are lane 1 as well: the stage in front of a product stage
    for s in up + dn:
        assert (sum(hints[s - 1]) > 0) == (lane1(s) > 0), s
    # against the rule over the Python mirror's tree: 23 cliques in the up pass, 2 in the down pass, and per time step the
    # updates they hold
    tree = iif.buildTreeReset(fg, order)
    tp = iif.TreeProgram(fg, tree, seed=1)
    (uside, ucount, uheld), (dside, dcount, dheld) = _rule(tp, tree)
    assert len(uside) == 23 and len(dside) == 2, (len(uside), len(dside))
    assert [len(hints[s]) for s in up] == ucount and [lane1(s) for s in up] == uheld
    assert [len(hints[s]) for s in dn] == [c for c in dcount if c] and [lane1(s) for s in dn] == [h for c, h in zip(dcount, dheld) if c]
