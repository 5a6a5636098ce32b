#!/usr/bin/env python3
"""Wall clock of the incremental loop (solve, add a pose, solve again): solveTree(fg, oldtree=tree) against SolveSession.solve().

A Euclid(2) chain at N particles grows one pose per step from --n0 to --n1 poses, eliminationOrder = fg.ls(), once with fixed
lag --lag and once without.  Two twin graphs are solved at every step, alternating which goes first:

  (a) tree = solveTree(fa, oldtree=tree)   -- a context per solve (and one more for graph initialisation), every belief up,
                                               every updated belief down
  (b) ses.solve() on fb                     -- one context, the beliefs resident

The per-step wall clock (a host clock around a call that ends in a device synchronise and the read-back) and the phases of
`return_timing` are taken over the last --last steps; the steps before them warm both legs up.  At the end the two graphs are
compared belief by belief (Euclid: bit-identical by contract).  Needs a GPU: there is no fallback.

  python tools/measure_incremental.py --out profiles/incremental_solve.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import iif_amd_loader  # noqa: E402

iif = iif_amd_loader.load()

PHASES_A = ("init_s", "tree_s", "compile_s", "solve_s")  # solveTree: compile_s holds the upload, the read-back is in the rest
PHASES_B = ("init_s", "tree_s", "compile_s", "upload_s", "solve_s", "readback_s")


def add_pose(fg):
    i = len(fg.ls())
    iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
    iif.addFactor(fg, [f"x{i - 1}", f"x{i}"], iif.LinearRelative(iif.MvNormal([1.0, 1.0], [0.1, 0.1])))


def stat(xs, scale=1e3):
    return f"median {statistics.median(xs) * scale:8.3f}  min {min(xs) * scale:8.3f}  max {max(xs) * scale:8.3f}"


def run_setting(lag, a, out):
    fa = iif.generateChainEuclid(a.n0, vardims=2, priorEvery=a.prior_every, N=a.N)
    fb = iif.generateChainEuclid(a.n0, vardims=2, priorEvery=a.prior_every, N=a.N)
    if lag:
        for fg in (fa, fb):
            iif.defaultFixedLagOnTree(fg, lag)
    ses = iif.SolveSession(fb, backend=a.make, reserve=a.reserve)
    tree = [None]
    rows_a, rows_b, traffic = [], [], []

    def leg_a(seed):
        t = time.perf_counter()
        tree[0], tm = iif.solveTree(fa, eliminationOrder=fa.ls(), backend=a.make, seed=seed, oldtree=tree[0], return_timing=True)
        tm["wall_s"] = time.perf_counter() - t
        return tm

    def leg_b(seed):
        t = time.perf_counter()
        _, tm = ses.solve(eliminationOrder=fb.ls(), seed=seed, return_timing=True)
        tm["wall_s"] = time.perf_counter() - t
        return tm

    try:
        leg_a(1), leg_b(1)  # the first solve of the n0-pose chain: graph initialisation of everything
        for step in range(a.n0, a.n1):
            add_pose(fa), add_pose(fb)
            if step % 2 == 0:
                ta, tb = leg_a(step), leg_b(step)
            else:
                tb, ta = leg_b(step), leg_a(step)
            rows_a.append(ta), rows_b.append(tb), traffic.append(dict(ses.stats["last"]))
        stats = {k: v for k, v in ses.stats.items() if k != "last"}
    finally:
        ses.close()
    same = all(np.array_equal(fa.getVal(v), fb.getVal(v)) and np.array_equal(fa.getVariable(v).bw, fb.getVariable(v).bw) for v in fa.ls())
    last = a.last
    A, B, tr = rows_a[-last:], rows_b[-last:], traffic[-last:]
    name = f"fixed lag {lag}" if lag else "no fixed lag"
    out(f"== {name}: chain {a.n0} -> {a.n1} poses, N = {a.N}; per-step figures over the last {len(A)} steps, ms ==")
    wa, wb = [r["wall_s"] for r in A], [r["wall_s"] for r in B]
    out(f"(a) solveTree(oldtree)   wall  {stat(wa)}")
    out(f"(b) SolveSession.solve   wall  {stat(wb)}")
    verdict = "the ranges do not overlap" if max(wb) < min(wa) else "THE RANGES OVERLAP"
    out(f"medians {statistics.median(wa) * 1e3:.3f} -> {statistics.median(wb) * 1e3:.3f} ms "
        f"({(statistics.median(wb) / statistics.median(wa) - 1) * 100:+.1f} %); {verdict} "
        f"(slowest (b) step {max(wb) * 1e3:.3f}, fastest (a) step {min(wa) * 1e3:.3f})")
    d = sorted(x - y for x, y in zip(wa, wb))  # the two legs solved the same graph at the same step
    out(f"paired, (a) - (b) at the same step: median {statistics.median(d) * 1e3:.3f}  min {d[0] * 1e3:.3f}  max {d[-1] * 1e3:.3f}; "
        f"(b) faster in {sum(x > 0 for x in d)} of {len(d)} steps; 10th .. 90th percentile of the wall clock: "
        f"(a) {sorted(wa)[len(wa) // 10] * 1e3:.3f} .. {sorted(wa)[-1 - len(wa) // 10] * 1e3:.3f}, "
        f"(b) {sorted(wb)[len(wb) // 10] * 1e3:.3f} .. {sorted(wb)[-1 - len(wb) // 10] * 1e3:.3f}")
    slow = max(range(len(B)), key=lambda i: wb[i])
    out(f"the slowest (b) step ({a.n1 - len(B) + slow} poses): " + ", ".join(f"{k} {B[slow][k] * 1e3:.3f}" for k in PHASES_B)
        + f", uploads {tr[slow]['uploads']}, resyncs {tr[slow]['resyncs']}")
    out("phases of return_timing:")
    for k in PHASES_A:
        out(f"  (a) {k:11s} {stat([r[k] for r in A])}" + ("   (graph + plan + context + upload of every belief + program)" if k == "compile_s" else ""))
    out(f"  (a) {'rest':11s} {stat([r['wall_s'] - sum(r[k] for k in PHASES_A) for r in A])}   (read-back, PPE, context teardown)")
    for k in PHASES_B:
        out(f"  (b) {k:11s} {stat([r[k] for r in B])}")
    out(f"  (b) {'rest':11s} {stat([r['wall_s'] - sum(r[k] for k in PHASES_B) for r in B])}")
    out(f"work per step (last step): cliques {B[-1]['cliques']}, updates up {B[-1]['updates_up']} / down {B[-1]['updates_down']}, "
        f"stages {B[-1]['stages']}, slots {B[-1]['slots']}; (a) the same: "
        f"{all(ra[k] == rb[k] for ra, rb in zip(A, B) for k in ('updates_up', 'updates_down', 'stages', 'slots'))}")
    nv = a.n1
    out(f"beliefs moved per step by (b): uploads median {statistics.median(t['uploads'] for t in tr):g} "
        f"(min {min(t['uploads'] for t in tr)}, max {max(t['uploads'] for t in tr)}), read-backs median "
        f"{statistics.median(t['readbacks'] for t in tr):g} (min {min(t['readbacks'] for t in tr)}, max {max(t['readbacks'] for t in tr)}); "
        f"(a) uploads every belief twice on a step with a new pose (initialisation, then the tree: {nv - last} .. {nv} each) and reads "
        f"the same updated beliefs back")
    out(f"session stats at the end: {stats}")
    out(f"beliefs of (a) and (b) after the last step: {'bit-identical' if same else 'DIFFERENT'}")
    out("")
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--n0", type=int, default=100)
    ap.add_argument("--n1", type=int, default=200)
    ap.add_argument("--last", type=int, default=50)
    ap.add_argument("--lag", type=int, default=30)
    ap.add_argument("--prior-every", type=int, default=100)
    ap.add_argument("--reserve", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backend", choices=("hip", "oracle"), default="hip",
                    help="oracle: the CPU checker, to rehearse the script where there is no GPU -- its times say nothing")
    a = ap.parse_args()
    a.make = None
    if a.backend == "oracle":
        from oracle.oracle_backend import OracleBackend
        a.make = lambda N, n_slots, side_ints=0: OracleBackend(N, n_slots, side_ints, threads=8)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("Incremental loop (solve, add a pose, solve again): solveTree(fg, oldtree=tree) against SolveSession.solve()")
    out("tools/measure_incremental.py; both legs in one process on one GPU, alternating which goes first at every step;")
    out("wall = host clock around one call (it ends in a device synchronise and the read-back of the results)")
    if a.backend != "hip":
        out("REHEARSAL on the CPU checker: the times below say nothing about the GPU")
    out("")
    ok = True
    for lag in (a.lag, 0):
        ok &= run_setting(lag, a, out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
