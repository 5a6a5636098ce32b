"""Time nbp_run_modes on resident beliefs beside what a caller has to do without it: read the beliefs back (beliefs_read) and
find the modes on the host (modes_numpy).  1, 100 and 1000 beliefs at N = 200 on Euclid(2) and SE(2); belief k is a mixture of
1 + k % 3 clusters, its bandwidth fitted on the device (nbp_run_bandwidth), the options the defaults (scale 2).  Host clock around
calls that end in a stream synchronise; the legs alternate in one process, every shape warmed up first.  The host route INCLUDES the
read-back it needs.  The figures of profiles/belief_modes.txt.

    python tools/measure_modes.py [--N 200] [--reps 20] [--host-reps 3] [--out FILE]
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
modes = iif.modes


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:64s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def belief(man, k, N, rng):
    """host points of belief k: 1 + k % 3 clusters, 2.0 apart with sigma 0.3 (the heading of SE(2): 1.0 apart, sigma 0.15)"""
    D = abi.MANIFOLD_DIM[man]
    which = rng.integers(1 + k % 3, size=N)
    X = rng.normal(0, 0.3, (N, D)) + 2.0 * which[:, None] + rng.normal(0, 1, D)[None, :]
    if man == abi.SE2:
        th = rng.normal(0, 0.15, N) + 1.0 * which
        return np.stack([X[:, 0], X[:, 1], np.cos(th), np.sin(th), -np.sin(th), np.cos(th)], axis=1)
    return X


def measure(man, name, n, N, reps, host_reps, out):
    be = iif.HipBackend(N, n)
    rng = np.random.default_rng(n)
    slots, mans = list(range(n)), [man] * n
    be.beliefs_write(slots, mans, [(belief(man, k, N, rng), None, None) for k in range(n)])
    be.run_bandwidth(slots, mans)
    for _ in range(3):  # warm-up: every shape of the timed window
        be.run_modes(slots, mans)
        be.beliefs_read(slots, mans)
    T = {k: [] for k in ("modes", "read", "numpy")}
    for r in range(reps):
        t, res = timed(lambda: be.run_modes(slots, mans))
        T["modes"].append(t)
        if r < host_reps:
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            T["read"].append((time.perf_counter() - t0) * 1e3)
            ref = [modes.modes_numpy(man, p, bw) for p, bw, _ in back]
            T["numpy"].append((time.perf_counter() - t0) * 1e3)
            # the two routes give the same answer (the criteria of tests/modes_cases.py; here: the discrete part)
            assert all(ref[i].n_modes == res[1][i] and np.array_equal(ref[i].labels, res[2][i]) for i in range(n))
    be.close()
    its, nm = res[3], res[1]
    out += [f"## {n} resident {name} belief{'s' if n > 1 else ''}: iterations per start median {int(np.median(its))}, max {int(its.max())}, "
            f"{int(its.sum())} in all ({int(its.sum()) * N / 1e6:.1f} M kernel terms); modes per belief 1: {int((nm == 1).sum())}, "
            f"2: {int((nm == 2).sum())}, 3: {int((nm == 3).sum())}, more: {int((nm > 3).sum())}; unconverged starts {int(res[4].sum())}",
            line("device: run_modes (one launch, one copy back)", T["modes"]),
            line("host route: beliefs_read of the same slots", T["read"]),
            line("host route: beliefs_read + modes_numpy of every belief", T["numpy"])]
    return np.median(T["modes"]), np.median(T["numpy"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--beliefs", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = [f"# nbp_run_modes beside the host route, N = {args.N}, the default options (bw_scale 2, tol 1e-6, max_iter 500, merge 1e-2), one "
           "MI355X; host clock around each call (the device calls end in a stream synchronise); median [min, max]; the legs alternate in "
           "one process, 3 warm-up rounds first.  Kernel times under rocprofv3 not taken."]
    print(out[0], flush=True)
    for man, name in ((abi.EUCLID2, "Euclid(2)"), (abi.SE2, "SE(2)")):
        for n in args.beliefs:
            d, h = measure(man, name, n, args.N, args.reps, min(args.host_reps, 1 if n >= 1000 else args.host_reps), out)
            out.append(f"host route / device: {h / d:.1f}")
            print("\n".join(out[-5:]), flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
