"""Time the belief overlaps on resident beliefs: nbp_run_overlap on 1, 1000 and 10 000 listed pairs (Euclid(2), and SE(2) masked to x-y
against Euclid(2) landmarks) at N = 200, and SolveSession.findOverlaps() on a 1000-pose and a 10 000-pose Euclid(2) chain after a
solve, beside the two routes a caller has without the search: read the beliefs back (beliefs_read) and search on the host
(overlap_search_numpy, the read-back included), and the device's own exhaustive route (run_overlap on all V (V - 1) / 2 pairs, or on
as many as --exhaustive-cap allows, extrapolated and marked as such).  n_evaluated / (V - 1) stands beside each search time.  Host
clock around calls that end in a stream synchronise; the legs alternate in one process, every shape warmed up first.  The figures of
profiles/belief_overlap.txt.

    python tools/measure_overlap.py [--N 200] [--reps 20] [--poses 1000 10000] [--exhaustive-cap 500000] [--out FILE]
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
ov = iif.overlap


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:86s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def se2_points(X):
    c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
    return np.stack([X[:, 0], X[:, 1], c, s, -s, c], axis=1)


def pair_form(N, reps, out):
    """nbp_run_overlap: 64 resident beliefs of each kind, pairs listed over them"""
    rng = np.random.default_rng(1)
    be = iif.HipBackend(N, 128)
    mans = [abi.EUCLID2] * 64 + [abi.SE2] * 64
    bels = [(rng.normal([0.3 * k, 0.0], 0.3, (N, 2)), [0.1, 0.1], None) for k in range(64)]
    bels += [(se2_points(np.c_[rng.normal([0.3 * k, 0.1], 0.3, (N, 2)), rng.uniform(-np.pi, np.pi, N)]), [0.1, 0.1, 0.2], None) for k in range(64)]
    be.beliefs_write(list(range(128)), mans, bels)
    for name, first_a, man_a in (("Euclid(2) against Euclid(2)", 0, abi.EUCLID2), ("SE(2) masked to x-y against Euclid(2)", 64, abi.SE2)):
        for n in (1, 1000, 10000):
            k = np.arange(n)
            cols = (list(first_a + k % 64), list((k * 7 + 1) % 64), [man_a] * n, [abi.EUCLID2] * n, [3] * n, [3] * n)
            for _ in range(3):
                be.run_overlap(*cols)
            T = [timed(lambda: be.run_overlap(*cols))[0] for _ in range(reps)]
            out.append(line(f"run_overlap, {n} pair{'s' if n > 1 else ''}, {name} (one launch, one copy back)", T))
            out.append(f"    {np.median(T) / n * 1e3:.2f} us per pair; {3 * 2 * N * N * n / 1e6:.1f} M kernel terms")
            print("\n".join(out[-2:]), flush=True)
    be.close()


def chain(V, N, reps, host_reps, cap, out):
    fg = iif.generateChainEuclid(V, vardims=2, priorEvery=max(V // 20, 1), N=N)
    with iif.SolveSession(fg) as ses:
        t, _ = timed(lambda: ses.solve(seed=1))
        out.append(f"## {V}-pose Euclid(2) chain, N = {N}, after a solve ({t:.0f} ms)")
        before = dict(ses.stats)
        for _ in range(2):
            got = ses.findOverlaps()
        T = {"search": [], "host": [], "read": []}
        be, labels = ses._be, list(ses._labels)
        slots, mans = list(range(len(labels))), [abi.EUCLID2] * len(labels)
        for r in range(reps):
            t, got = timed(ses.findOverlaps)
            T["search"].append(t)
            if r < host_reps:
                t0 = time.perf_counter()
                back = be.beliefs_read(slots, mans)
                T["read"].append((time.perf_counter() - t0) * 1e3)
                ref = ov.overlap_search_numpy([(abi.EUCLID2, p, bw, 3) for p, bw, _ in back], N=N)
                T["host"].append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(ref[0], got.idx) and np.array_equal(ref[2], [got.n_found[v] for v in labels])
                assert np.array_equal(ref[3], [got.n_evaluated[v] for v in labels])
        assert {k: ses.stats[k] for k in ("uploads", "readbacks")} == {k: before[k] for k in ("uploads", "readbacks")}
        ev = np.array([got.n_evaluated[v] for v in labels])
        out.append(f"    n_evaluated / (V - 1): mean {ev.mean() / (V - 1):.5f}, max {ev.max() / (V - 1):.5f} ({int(ev.sum())} ordered pairs of "
                   f"{V * (V - 1)} evaluated); partners found per pose: median {int(np.median([got.n_found[v] for v in labels]))}; {len(got.pairs())} unique pairs")
        out.append(line("device: ses.findOverlaps() (two launches, one copy back, no belief moves)", T["search"]))
        out.append(line("host route: beliefs_read of the same slots", T["read"]))
        out.append(line("host route: beliefs_read + overlap_search_numpy (the same box rule)", T["host"]))
        # the device's own exhaustive route
        ii, jj = np.triu_indices(V, 1)
        total = len(ii)
        n = min(total, cap)
        cols = (list(ii[:n]), list(jj[:n]), [abi.EUCLID2] * n, [abi.EUCLID2] * n, [3] * n, [3] * n)
        be.run_overlap(*cols)
        E = [timed(lambda: be.run_overlap(*cols))[0] for _ in range(max(3, min(reps, 5)))]
        if n == total:
            out.append(line(f"device, exhaustive: run_overlap on all {total} pairs", E))
            ex = np.median(E)
        else:
            ex = np.median(E) * total / n
            out.append(line(f"device, exhaustive: run_overlap on the first {n} of {total} pairs", E))
            out.append(f"    EXTRAPOLATED to all {total} pairs (x {total / n:.1f}): {ex:.0f} ms -- not measured")
        out.append(f"    exhaustive / search: {ex / np.median(T['search']):.1f}; host route / search: {np.median(T['host']) / np.median(T['search']):.1f}")
    print("\n".join(out[-8:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--poses", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--exhaustive-cap", type=int, default=500000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = [f"# belief overlaps on resident beliefs, N = {args.N}, the default options (reach 6, min_coeff 1e-3, topk 8), one MI355X; host clock "
           "around each call (the device calls end in a stream synchronise, the read-back of the results included); median [min, max]; "
           "3 warm-up rounds first.  Kernel times under rocprofv3 not taken."]
    print(out[0], flush=True)
    pair_form(args.N, args.reps, out)
    for V in args.poses:
        chain(V, args.N, args.reps, args.host_reps, args.exhaustive_cap, out)
    text = "\n".join(out) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
