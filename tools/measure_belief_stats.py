"""Time nbp_run_meancov and nbp_run_kld on resident beliefs beside what a caller had to do without them: read the beliefs back
(beliefs_read) and compute on the host (meancov_numpy / kld_numpy).  1000 Euclid(2) beliefs at N = 200 -- the size of
profiles/ppe_kernel.txt; the kld of each belief against its neighbour.  Host clock around calls that end in a stream synchronise;
the legs alternate in one process.  The figures of profiles/belief_stats_kernels.txt.

    python tools/measure_belief_stats.py [--beliefs 1000] [--reps 20] [--host-reps 3] [--out FILE]
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
bs = iif.beliefstats


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:58s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beliefs", type=int, default=1000)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, N, man = args.beliefs, args.N, abi.EUCLID2
    be = iif.HipBackend(N, n)
    rng = np.random.default_rng(0)
    slots, mans = list(range(n)), [man] * n
    for a in range(0, n, 500):
        b = min(a + 500, n)
        be.beliefs_write(slots[a:b], mans[a:b], [(rng.normal(rng.normal(0, 1, 2), 0.5, (N, 2)), None, None) for _ in range(a, b)])
    be.run_bandwidth(slots, mans)
    nb = slots[1:] + slots[:1]  # each belief's neighbour
    for _ in range(3):  # warm-up: every shape of the timed window
        be.run_meancov(slots, mans)
        be.run_kld(slots, nb, mans)
        be.beliefs_read(slots, mans)
    T = {k: [] for k in ("meancov", "kld", "read", "np_meancov", "np_kld")}
    for r in range(args.reps):
        t, (mean, cov) = timed(lambda: be.run_meancov(slots, mans))
        T["meancov"].append(t)
        t, val = timed(lambda: be.run_kld(slots, nb, mans))
        T["kld"].append(t)
        t, back = timed(lambda: be.beliefs_read(slots, mans))
        T["read"].append(t)
        if r < args.host_reps:
            t, ref = timed(lambda: [bs.meancov_numpy(man, p) for p, _, _ in back])
            T["np_meancov"].append(t)
            t, kref = timed(lambda: [bs.kld_numpy(man, back[i][0], back[i][1], back[j][0], back[j][1]) for i, j in zip(slots, nb)])
            T["np_kld"].append(t)
            # the two routes give the same numbers (the criteria of tests/stats_cases.py; here: a plain sanity bound)
            assert max(np.abs(cov[i, :2, :2] - ref[i][1]).max() for i in range(n)) < 1e-12
            assert max(abs(val[i] - kref[i]) / (1 + abs(kref[i])) for i in range(n)) < 1e-9
    be.close()
    out = [f"# {n} resident Euclid(2) beliefs, N = {N}, one MI355X; host clock around each call (the device calls end in a stream "
           f"synchronise); median [min, max]; the legs alternate in one process, 3 warm-up rounds first",
           line("device: run_meancov (one launch, 12 doubles per belief back)", T["meancov"]),
           line("device: run_kld, each belief against its neighbour", T["kld"]),
           line("host route: beliefs_read of the same slots", T["read"]),
           line("host route: + meancov_numpy of every belief", T["np_meancov"]),
           line("host route: + kld_numpy of every pair", T["np_kld"])]
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
