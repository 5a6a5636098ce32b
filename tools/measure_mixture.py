"""Time the mixture summary of resident beliefs (nbp_run_modes for the start, then nbp_run_mixture) beside what a caller has to do
without it: read the beliefs back (beliefs_read), find the modes on the host (modes_numpy) and run the EM there (mixture_numpy).
1, 100 and 1000 beliefs at N = 200 on Euclid(2) and SE(2); belief k is a mixture of 1 + k % 3 clusters 1.2 apart with sigma 0.3
(neighbours overlap), its bandwidth fitted on the device (nbp_run_bandwidth), the options the defaults (at most 8 components, scale
2, tol 1e-8, max_iter 500).  Host clock around calls that end in a stream synchronise; the legs alternate in one process, every
shape warmed up first.  The host route INCLUDES the read-back it needs.  The figures of profiles/belief_mixture.txt.

    python tools/measure_mixture.py [--N 200] [--reps 20] [--host-reps 3] [--out FILE]
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
mixture = iif.mixture


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:72s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def belief(man, k, N, rng):
    """host points of belief k: 1 + k % 3 clusters, 1.2 apart with sigma 0.3 (the heading of SE(2): 0.6 apart, sigma 0.15)"""
    D = abi.MANIFOLD_DIM[man]
    which = rng.integers(1 + k % 3, size=N)
    X = rng.normal(0, 0.3, (N, D)) + 1.2 * which[:, None] + rng.normal(0, 1, D)[None, :]
    if man == abi.SE2:
        th = rng.normal(0, 0.15, N) + 0.6 * which
        return np.stack([X[:, 0], X[:, 1], np.cos(th), np.sin(th), -np.sin(th), np.cos(th)], axis=1)
    return X


def measure(man, name, n, N, reps, host_reps, out):
    be = iif.HipBackend(N, n)
    rng = np.random.default_rng(n)
    slots, mans, counts = list(range(n)), [man] * n, [N] * n
    K, mode_kw, kw = mixture._options(abi.MIX_MAX, abi.MODES_BW_SCALE, abi.MIX_TOL, abi.MIX_MAX_ITER)
    be.beliefs_write(slots, mans, [(belief(man, k, N, rng), None, None) for k in range(n)])
    be.run_bandwidth(slots, mans)
    # the start of the EM alone, for the leg that times nbp_run_mixture by itself
    res = be.run_modes(slots, mans, **mode_kw)
    lab, mu = np.full((n, N), -1, dtype=np.int32), np.zeros((n, abi.MIX_MAX, abi.MAXD))
    for i in range(n):
        lab[i], mu[i] = mixture.starting_from_modes(iif.modes.modes_from_records(man, *(r[i] for r in res), N), K)
    for _ in range(3):  # warm-up: every shape of the timed window
        mixture.resident_mixtures(be, slots, mans, counts, K, mode_kw, kw)
        be.run_mixture(slots, mans, lab, mu, **kw)
        be.beliefs_read(slots, mans)
    T = {k: [] for k in ("query", "em", "read", "numpy")}
    for r in range(reps):
        t, got = timed(lambda: mixture.resident_mixtures(be, slots, mans, counts, K, mode_kw, kw))
        T["query"].append(t)
        t, (recs, _) = timed(lambda: be.run_mixture(slots, mans, lab, mu, **kw))
        T["em"].append(t)
        if r < host_reps:
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            T["read"].append((time.perf_counter() - t0) * 1e3)
            ref = [mixture.mixture_host(man, p, bw, K, mode_kw, kw) for p, bw, _ in back]
            T["numpy"].append((time.perf_counter() - t0) * 1e3)
            # do the two routes give the same answer?  (The criteria are those of tests/mixture_cases.py; here: a count.)
            same = sum(ref[i].n_comp == got[i].n_comp and abs(ref[i].iters - got[i].iters) <= 1 and
                       np.abs(ref[i].weights - got[i].weights).max() <= 1e-6 for i in range(n))
    be.close()
    its, nc = recs["iters"], recs["n_comp"]
    out += [f"## {n} resident {name} belief{'s' if n > 1 else ''}: EM iterations per belief median {int(np.median(its))}, slowest {int(its.max())}, "
            f"{int(its.sum())} in all; components per belief 1: {int((nc == 1).sum())}, 2: {int((nc == 2).sum())}, 3: {int((nc == 3).sum())}, "
            f"more: {int((nc > 3).sum())}; dropped {int(recs['n_dropped'].sum())}; stopped at max_iter {int((recs['converged'] == 0).sum())}; "
            f"the host route agrees (components, iterations +-1, weights to 1e-6) on {same} of {n}",
            line("device: run_modes + run_mixture (two launches, the labels through the host)", T["query"]),
            line("device: run_mixture alone (one launch, one copy each way)", T["em"]),
            line("host route: beliefs_read of the same slots", T["read"]),
            line("host route: beliefs_read + modes_numpy + mixture_numpy of every belief", T["numpy"])]
    return np.median(T["query"]), np.median(T["numpy"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--beliefs", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = [f"# the mixture summary of resident beliefs beside the host route, N = {args.N}, the default options (at most 8 components, "
           "bw_scale 2, tol 1e-8, max_iter 500), one MI355X; host clock around each call (the device calls end in a stream synchronise); "
           "median [min, max]; the legs alternate in one process, 3 warm-up rounds first.  Kernel times under rocprofv3 not taken."]
    print(out[0], flush=True)
    for man, name in ((abi.EUCLID2, "Euclid(2)"), (abi.SE2, "SE(2)")):
        for n in args.beliefs:
            d, h = measure(man, name, n, args.N, args.reps, min(args.host_reps, 1 if n >= 1000 else args.host_reps), out)
            out.append(f"host route / device: {h / d:.1f}")
            print("\n".join(out[-6:]), flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
