"""Time nbp_run_factor_likelihood on resident beliefs beside the two routes a caller has without it: read the beliefs back
(beliefs_read) and evaluate the definition on the host (factor_likelihood_numpy), and -- for 100 factors -- the existing
approxDeconv + mmd, one factor at a time.  1, 100, 1000 and 10 000 factors at N = 200: a chain of poses on Euclid(2) with
LinearRelative factors, and on SE(2) with ManifoldFactor factors; factor k joins the beliefs in slots k and k + 1.  Host clock
around calls that end in a stream synchronise; the legs alternate in one process, every shape warmed up first.  The host routes
INCLUDE the read-back they need.  A second table splits the single-item call into its launch + copies and its kernel: the same call
on beliefs of 8 points in the same context (64 pair terms instead of 40 000) is all overhead.  The figures of
profiles/factor_likelihood.txt.

    python tools/measure_factor_likelihood.py [--N 200] [--reps 20] [--host-reps 3] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import iif_amd_loader  # noqa: E402

iif = iif_amd_loader.load()
abi = iif.abi
lik = iif.likelihood

L3 = np.diag([0.1, 0.1, 0.05])
MODELS = {
    abi.EUCLID2: ("Euclid(2) LinearRelative", abi.F_LINREL, [(1.0, [1.0, 0.0], np.diag([0.1, 0.1]))],
                  lambda: iif.LinearRelative(iif.MvNormal([1.0, 0.0], [0.1, 0.1])), iif.ContinuousEuclid(2)),
    abi.SE2: ("SE(2) ManifoldFactor", abi.F_SE2, [(1.0, [1.0, 0.0, 0.1], L3)],
              lambda: iif.ManifoldFactor(iif.MvNormal([1.0, 0.0, 0.1], L3 @ L3.T)), iif.SpecialEuclidean2),
}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:72s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def pose(man, k, n, rng):
    """host points of pose k of the chain: one unit along x per pose, heading 0.1 k, sigma 0.1 (heading 0.05)"""
    th = 0.1 * k
    if man == abi.SE2:
        x = np.cumsum(np.cos(0.1 * np.arange(k + 1)))[-1] - 1.0 + rng.normal(0, 0.1, n)
        y = np.cumsum(np.sin(0.1 * np.arange(k + 1)))[-1] + rng.normal(0, 0.1, n)
        t = th + rng.normal(0, 0.05, n)
        return np.stack([x, y, np.cos(t), np.sin(t), -np.sin(t), np.cos(t)], axis=1)
    return rng.normal([float(k), 0.0], 0.1, (n, 2))


def measure(man, n, N, reps, host_reps, out):
    name, kind, comps, make, vt = MODELS[man]
    be = iif.HipBackend(N, n + 1)
    rng = np.random.default_rng(n)
    slots, mans = list(range(n + 1)), [man] * (n + 1)
    pts = [pose(man, k % 50, N, rng) for k in range(n + 1)]
    be.beliefs_write(slots, mans, [(p, None, None) for p in pts])
    descs = (abi.LikelihoodDesc * n)(*[lik.likelihood_desc(kind, man, comps, 0, k, k + 1) for k in range(n)])
    for _ in range(3):  # warm-up: every shape of the timed window
        be.run_factor_likelihood(descs)
        be.beliefs_read(slots, mans)
    T = {k: [] for k in ("device", "read", "numpy", "deconv")}
    worst = 0.0
    for r in range(reps):
        t, (ll, cl) = timed(lambda: be.run_factor_likelihood(descs))
        T["device"].append(t)
        if r < host_reps:
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            T["read"].append((time.perf_counter() - t0) * 1e3)
            ref = [lik.factor_likelihood_numpy(descs[k], back[k][0], back[k + 1][0])[0] for k in range(n)]
            T["numpy"].append((time.perf_counter() - t0) * 1e3)
            worst = max(worst, float(np.abs((np.array(ref) - ll) / np.maximum(1.0, np.abs(ref))).max()))
    out += [f"## {n} {name} factor{'s' if n > 1 else ''} on resident beliefs ({N * N * n / 1e6:.2f} M pair terms); device against the host "
            f"route: largest difference {worst:.1e} relative",
            line("device: run_factor_likelihood (one upload, one launch, one copy back)", T["device"]),
            line("host route: beliefs_read of the same slots", T["read"]),
            line("host route: beliefs_read + factor_likelihood_numpy of every factor", T["numpy"])]
    if n == 100:  # what the library offered before: approxDeconv (a search per particle) + mmd, one factor at a time
        fg = iif.initfg(iif.SolverParams(N=N))
        for k in range(n + 1):
            iif.addVariable(fg, f"x{k}", vt)
        for k in range(n):
            iif.addFactor(fg, [f"x{k}", f"x{k + 1}"], make(), label=f"f{k}")
        dbe = iif.HipBackend(N, 4)
        zman = abi.EUCLID2 if man == abi.EUCLID2 else abi.EUCLID3
        for r in range(min(host_reps, 2)):
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            for k in range(n + 1):
                iif.setValKDE(fg, f"x{k}", back[k][0], back[k][1])
            for k in range(n):
                pred, meas = iif.approxDeconv(fg, f"f{k}", backend=dbe, seed=k)
                iif.mmd_numpy(zman, pred, meas)
            T["deconv"].append((time.perf_counter() - t0) * 1e3)
        dbe.close()
        out.append(line("old route: beliefs_read + approxDeconv (device) + mmd (host) per factor", T["deconv"]))
    be.close()
    return np.median(T["device"]), np.median(T["numpy"])


def overhead(man, N, reps, out):
    """one item on beliefs of N points and on beliefs of 8 points in the same context: the second is launch + copies alone"""
    name, kind, comps, _, _ = MODELS[man]
    be = iif.HipBackend(N, 4)
    rng = np.random.default_rng(1)
    bw = np.ones(abi.MANIFOLD_DIM[man])  # (never read by the query; a belief of fewer than N points must bring one)
    be.beliefs_write([0, 1, 2, 3], [man] * 4, [(pose(man, 0, N, rng), bw, None), (pose(man, 1, N, rng), bw, None),
                                               (pose(man, 0, 8, rng), bw, None), (pose(man, 1, 8, rng), bw, None)])
    full, tiny = lik.likelihood_desc(kind, man, comps, 0, 0, 1), lik.likelihood_desc(kind, man, comps, 0, 2, 3)
    for _ in range(5):
        be.run_factor_likelihood([full])
        be.run_factor_likelihood([tiny])
    T = {"full": [], "tiny": []}
    for _ in range(reps):
        T["full"].append(timed(lambda: be.run_factor_likelihood([full]))[0])
        T["tiny"].append(timed(lambda: be.run_factor_likelihood([tiny]))[0])
    be.close()
    f, t = np.median(T["full"]), np.median(T["tiny"])
    out += [f"## one {name} item: where the time goes",
            line(f"one item, beliefs of {N} points ({N * N} pair terms)", T["full"]),
            line("one item, beliefs of 8 points (64 pair terms): upload + launch + copy back", T["tiny"]),
            f"launch + copies: {100 * t / f:.0f} % of the single-item call, the kernel's pair loops the rest ({f - t:.3f} ms)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--factors", type=int, nargs="+", default=[1, 100, 1000, 10000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = [f"# nbp_run_factor_likelihood beside the host routes, N = {args.N}, one MI355X; host clock around each call (the device calls "
           "end in a stream synchronise); median [min, max]; the legs alternate in one process, 3 warm-up rounds first.  Kernel times under "
           "rocprofv3 not taken."]
    print(out[0], flush=True)
    for man in (abi.EUCLID2, abi.SE2):
        for n in args.factors:
            at = len(out)
            d, h = measure(man, n, args.N, args.reps, 1 if n >= 1000 else args.host_reps, out)
            out.append(f"host route / device: {h / d:.1f}")
            print("\n".join(out[at:]), flush=True)
        at = len(out)
        overhead(man, args.N, args.reps, out)
        print("\n".join(out[at:]), flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
