"""Time nbp_run_ppe beside nbp_run_bandwidth on the same resident beliefs (Euclid(2), N = 200): host clock around calls that end
in a stream synchronise, warm-up first, medians.  The figures of profiles/ppe_kernel.txt.

    python tools/ppe_bench.py [--reps 15] [--sizes 1,1000,10000]
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
    N, man = args.N, abi.EUCLID2
    be = iif.HipBackend(N, max(sizes))
    rng = np.random.default_rng(0)
    slots, mans = list(range(max(sizes))), [man] * max(sizes)
    for a in range(0, max(sizes), 500):
        b = min(a + 500, max(sizes))
        be.beliefs_write(slots[a:b], mans[a:b], [(rng.normal(rng.normal(0, 3, 2), 0.5, (N, 2)), None, None) for _ in range(a, b)])
    be.run_bandwidth(slots, mans)
    print(f"# Euclid(2) beliefs, N = {N}; host clock around the call (upload of the slot list, launch, copy back, synchronise); "
          f"median [min, max] of {args.reps} after 3 warm-up calls")
    for n in sizes:
        p = median_ms(lambda: be.run_ppe(slots[:n], mans[:n]), args.reps)
        f = median_ms(lambda: be.run_bandwidth(slots[:n], mans[:n]), args.reps)
        print(f"beliefs {n:6d}: nbp_run_ppe {p[0]:9.3f} ms [{p[1]:.3f}, {p[2]:.3f}]   nbp_run_bandwidth {f[0]:9.3f} ms [{f[1]:.3f}, {f[2]:.3f}]"
              f"   ppe / fit = {p[0] / f[0]:.3f}", flush=True)
    be.close()


if __name__ == "__main__":
    main()
