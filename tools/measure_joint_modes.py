"""Time the mode-by-mode factor likelihoods (nbp_run_factor_mode_likelihood) and the joint-hypothesis query built on them.
The figures of profiles/joint_modes.txt, at N = 200 on one MI355X.

(a) Kernel cost.  The grouped kernel at 1 / 100 / 1000 / 10 000 LinearRelative Euclid(2) and ManifoldFactor SE(2) items with
    1 x 1, 2 x 2 and 8 x 8 groups, beside nbp_run_factor_likelihood on the same items (the ungrouped kernel: the yardstick).  The
    pair loop is the same; the extra work is the stable sort of B into groups and one block reduction per present cell, pass and
    component.  Factor k joins the beliefs in slots k and k + 1; the items share sixteen label rows, so that the upload stays
    what it is for the ungrouped call (a second line gives the 2 x 2 call with one label row per belief: n + 1 rows go up).
(b) Query cost.  SolveSession.jointModes() on a 100-pose and a 1000-pose circular chain with door sightings, after a solve, beside
    the route a caller has without it: beliefs_read of every slot plus jointModes on the host copy (numpy), the read-back
    included.  The host elimination (joint_from_tables: the same on both routes) is reported separately.

Host clock around calls that end in a stream synchronise; medians of `--reps` with ranges; every shape warmed up first.  Every step
runs in a process of its own under its own time limit, and the steps after one that fails or runs out of time are not started.

    python tools/measure_joint_modes.py [--N 200] [--reps 20] [--limit 300] [--steps kernel:e2 ...] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

STEPS = ["kernel:e2", "kernel:se2", "query:100", "query:1000"]


def line(name, t):
    return f"{name:86s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def kernel_step(iif, which, N, reps, counts):
    abi, lik = iif.abi, iif.likelihood
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from measure_factor_likelihood import MODELS, pose
    man = abi.EUCLID2 if which == "e2" else abi.SE2
    name, kind, comps, _, _ = MODELS[man]
    out = []
    for n in counts:
        be = iif.HipBackend(N, n + 1)
        rng = np.random.default_rng(n)
        be.beliefs_write(list(range(n + 1)), [man] * (n + 1), [(pose(man, k % 50, N, rng), None, None) for k in range(n + 1)])
        descs = (abi.LikelihoodDesc * n)(*[lik.likelihood_desc(kind, man, comps, 0, k, k + 1) for k in range(n)])
        shared = {K: rng.integers(0, K, (16, N)).astype(np.int32) for K in (1, 2, 8)}
        own = rng.integers(0, 2, (n + 1, N)).astype(np.int32)
        ra, rb = [k % 16 for k in range(n)], [(k + 1) % 16 for k in range(n)]
        calls = {"plain": lambda: be.run_factor_likelihood(descs)}
        for K in (1, 2, 8):
            calls[f"{K}x{K}"] = lambda K=K: be.run_factor_mode_likelihood(descs, ra, rb, shared[K])
        calls["2x2 own rows"] = lambda: be.run_factor_mode_likelihood(descs, list(range(n)), list(range(1, n + 1)), own)
        for f in calls.values():
            for _ in range(3):
                f()
        T = {k: [] for k in calls}
        for _ in range(reps):  # the legs alternate
            for k, f in calls.items():
                T[k].append(timed(f)[0])
        ll = be.run_factor_likelihood(descs)[0]
        t1 = be.run_factor_mode_likelihood(descs, [-1] * n, [-1] * n, np.zeros((0, N), dtype=np.int32))[0]
        same = bool(np.array_equal(t1[:, 0, 0], ll))
        be.close()
        m = {k: float(np.median(v)) for k, v in T.items()}
        out += [f"## {n} {name} item{'s' if n > 1 else ''} ({N * N * n / 1e6:.2f} M pair terms); one group: T[0, 0] == loglik bit for bit: {same}",
                line("nbp_run_factor_likelihood (the ungrouped kernel)", T["plain"]),
                line("nbp_run_factor_mode_likelihood, 1 x 1 groups (1 cell: 1 block_max + 1 block_sum)", T["1x1"]),
                line("nbp_run_factor_mode_likelihood, 2 x 2 groups (4 cells)", T["2x2"]),
                line("nbp_run_factor_mode_likelihood, 8 x 8 groups (64 cells)", T["8x8"]),
                line(f"nbp_run_factor_mode_likelihood, 2 x 2 groups, one label row per belief ({(n + 1) * N * 4 / 1e3:.1f} kB more go up)", T["2x2 own rows"]),
                f"grouped / ungrouped: 1 x 1 {m['1x1'] / m['plain']:.2f}, 2 x 2 {m['2x2'] / m['plain']:.2f}, 8 x 8 {m['8x8'] / m['plain']:.2f}, "
                f"2 x 2 with own rows {m['2x2 own rows'] / m['plain']:.2f}"]
    return out


def query_step(iif, nposes, N, reps):
    jm = iif.jointmodes
    fg = iif.generateCircularDoors(nposes=nposes, N=N, sightEvery=25)
    out = []
    with iif.SolveSession(fg) as ses:  # (backend None: libnbp)
        t_solve, _ = timed(lambda: ses.solve(seed=5))
        before = dict(ses.stats)
        for _ in range(2):
            got = ses.jointModes()
        T = {k: [] for k in ("session", "modes", "elim", "read", "numpy")}
        for _ in range(reps):
            T["session"].append(timed(ses.jointModes)[0])
            T["modes"].append(timed(lambda: ses.getBeliefModes(list(got.modes)))[0])
            T["elim"].append(timed(lambda: jm.joint_from_tables(got.modes, got.tables, got.skipped))[0])
        assert {k: v for k, v in ses.stats.items() if k != "last"} == {k: v for k, v in before.items() if k != "last"}, "the query moved a belief"
        be = ses._be
        labels = list(got.modes)
        place = {v: i for i, v in enumerate(ses._labels)}
        slots, mans = [place[v] for v in labels], [fg.getVariable(v).varType.manifold for v in labels]
        ref = None
        for _ in range(1 if nposes >= 1000 else 2):
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            T["read"].append((time.perf_counter() - t0) * 1e3)
            for v, (pts, bw, _) in zip(labels, back):
                iif.setValKDE(fg, v, pts, bw)
            ref = iif.jointModes(fg)
            T["numpy"].append((time.perf_counter() - t0) * 1e3)
        agree = ref.best == got.best
        nmulti = len(got.variables)
        kmax = max(m.n_modes for m in got.modes.values())
    s, h = float(np.median(T["session"])), float(np.median(T["numpy"]))
    out += [f"## jointModes on a {nposes}-pose circular chain with door sightings every 25 poses ({len(got.tables)} factors, {len(got.modes)} "
            f"variables, {nmulti} of them multimodal, at most {kmax} modes; the solve before it {t_solve:.0f} ms); best joint hypothesis equal "
            f"on both routes: {agree}; best weight {got.best_weight:.6f}",
            line("SolveSession.jointModes(): run_modes + run_factor_mode_likelihood + host elimination", T["session"]),
            line("  of which SolveSession.getBeliefModes (one run_modes launch)", T["modes"]),
            line("  of which the host elimination (joint_from_tables, both semirings)", T["elim"]),
            line("host route: beliefs_read of the same slots", T["read"]),
            line("host route: beliefs_read + jointModes on the host copy (numpy)", T["numpy"]),
            f"host route / session: {h / s:.1f}"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--items", type=int, nargs="+", default=[1, 100, 1000, 10000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="run this one step in this process: " + ", ".join(STEPS))
    ap.add_argument("--steps", nargs="+", default=STEPS, help="the steps to run, each in a process of its own")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import iif_amd_loader
        iif = iif_amd_loader.load()
        kind, what = args.step.split(":")
        rows = kernel_step(iif, what, args.N, args.reps, args.items) if kind == "kernel" else query_step(iif, int(what), args.N, args.reps)
        print("\n".join(rows), flush=True)
        return 0
    out = [f"# nbp_run_factor_mode_likelihood beside nbp_run_factor_likelihood, and SolveSession.jointModes beside the host route; N = {args.N}, "
           f"one MI355X; host clock around each call (the device calls end in a stream synchronise); median [min, max] of {args.reps}; the "
           "legs alternate in one process, warm-up rounds first.  Kernel times under rocprofv3 not taken."]
    rc = 0
    for step in args.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--N", str(args.N), "--reps", str(args.reps), "--items"] + [str(i) for i in args.items]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out.append(f"## step {step}: ended at its time limit of {args.limit} s; the steps behind it were not started")
            rc = 124
            break
        out.append(p.stdout.rstrip())
        print(out[-1], flush=True)
        if p.returncode != 0:
            out.append(f"## step {step}: exit status {p.returncode}; the steps behind it were not started\n" + p.stderr[-2000:])
            rc = p.returncode
            break
    text = "\n".join(out) + "\n"
    print(text if rc else "", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
