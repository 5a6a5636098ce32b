"""Time nbp_run_mmd and nbp_run_evaluate (4 and 1000 queries per belief) beside nbp_run_ppe on the same resident beliefs
(Euclid(2), N = 200): host clock around calls that end in a stream synchronise, warm-up first, medians.  The figures of
profiles/query_kernels.txt.

    python tools/query_bench.py [--reps 15] [--sizes 1,1000,10000]
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


def median_ms(f, reps, warmup=3):
    for _ in range(warmup):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="1,1000,10000")
    ap.add_argument("--N", type=int, default=200)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    N, man, top = args.N, abi.EUCLID2, max(sizes)
    be = iif.HipBackend(N, 2 * top)  # beliefs i and top + i are the two sides of pair i (a solve's posterior and the previous one)
    rng = np.random.default_rng(0)
    slots, mans = list(range(2 * top)), [man] * (2 * top)
    for a in range(0, 2 * top, 500):
        b = min(a + 500, 2 * top)
        be.beliefs_write(slots[a:b], mans[a:b], [(rng.normal(rng.normal(0, 3, 2), 0.5, (N, 2)), None, None) for _ in range(a, b)])
    be.run_bandwidth(slots, mans)
    print(f"# Euclid(2) beliefs, N = {N}; host clock around the call (uploads, launch, copy back, synchronise; the Python wrapper's "
          f"packing of the queries included); median [min, max] of {args.reps} after 3 warm-up calls")
    for n in sizes:
        q4 = [rng.normal(0, 3, (4, 2)) for _ in range(n)]
        q1000 = [rng.normal(0, 3, (1000, 2)) for _ in range(n)]
        rows = [("nbp_run_ppe", lambda: be.run_ppe(slots[:n], mans[:n])),
                ("nbp_run_mmd", lambda: be.run_mmd(slots[:n], slots[top:top + n], mans[:n], 0.001)),
                ("nbp_run_evaluate 4 q", lambda: be.run_evaluate(slots[:n], mans[:n], q4)),
                ("nbp_run_evaluate 1000 q", lambda: be.run_evaluate(slots[:n], mans[:n], q1000))]
        for name, f in rows:
            t = median_ms(f, args.reps)
            print(f"beliefs {n:6d}: {name:24s} {t[0]:10.3f} ms [{t[1]:.3f}, {t[2]:.3f}]", flush=True)
    be.close()


if __name__ == "__main__":
    main()
