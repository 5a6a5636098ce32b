"""Time nbp_run_credible on resident beliefs beside what a caller has to do without it: read the beliefs back (beliefs_read) and
evaluate the definition on the host (credible_numpy); then the calibration of the solver's beliefs against a known truth.

Timings: 1, 100 and 1000 beliefs at N = 200 on Euclid(2) and SE(2); belief k is a mixture of 1 + k % 3 clusters, its bandwidth
fitted on the device (nbp_run_bandwidth); the default masses (0.5, 0.9, 0.95) and probabilities, the per-particle outputs asked for,
one reference point per belief.  Host clock around calls that end in a stream synchronise; the legs alternate in one process, every
shape warmed up first.  The host route INCLUDES the read-back it needs.

Calibration: the BASELINE config-2 chain of 100 Euclid(2) poses (generateGraph_LineStep through generateChainEuclid, one prior at
x0, truth x_i = (i, i)), solved in a SolveSession for 10 seeds; coverage(ses.credibility(truth)) at 0.5 / 0.9 / 0.95 per seed and
pooled, and the same by decade of poses.  Reported, not asserted: it is a finding about the solver.

The figures of profiles/belief_credible.txt.

    python tools/measure_credible.py [--N 200] [--reps 20] [--host-reps 3] [--seeds 10] [--out FILE]
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
cr = iif.credible


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def line(name, t):
    return f"{name:64s} {np.median(t):10.3f} ms [{min(t):.3f}, {max(t):.3f}] (n = {len(t)})"


def belief(man, k, N, rng):
    """host points of belief k and a reference point: 1 + k % 3 clusters, 2.0 apart with sigma 0.3 (the heading of SE(2): 1.0
    apart, sigma 0.15); the reference point is drawn from the same law"""
    D = abi.MANIFOLD_DIM[man]
    which = rng.integers(1 + k % 3, size=N + 1)
    X = rng.normal(0, 0.3, (N + 1, D)) + 2.0 * which[:, None] + rng.normal(0, 1, D)[None, :]
    if man == abi.SE2:
        X[:, 2] = rng.normal(0, 0.15, N + 1) + 1.0 * which
        th = X[:N, 2]
        return np.stack([X[:N, 0], X[:N, 1], np.cos(th), np.sin(th), -np.sin(th), np.cos(th)], axis=1), X[N:]
    return X[:N], X[N:]


def measure(man, name, n, N, reps, host_reps, out):
    be = iif.HipBackend(N, n)
    rng = np.random.default_rng(n)
    slots, mans = list(range(n)), [man] * n
    D = abi.MANIFOLD_DIM[man]
    masks = [(1 << D) - 1] * n
    made = [belief(man, k, N, rng) for k in range(n)]
    Qs = [q for _, q in made]
    be.beliefs_write(slots, mans, [(p, None, None) for p, _ in made])
    be.run_bandwidth(slots, mans)
    for _ in range(3):  # warm-up: every shape of the timed window
        be.run_credible(slots, mans, masks, cr.MASS, cr.PROBS, Qs)
        be.beliefs_read(slots, mans)
    T = {k: [] for k in ("credible", "read", "numpy")}
    agree = 0
    for r in range(reps):
        t, res = timed(lambda: be.run_credible(slots, mans, masks, cr.MASS, cr.PROBS, Qs))
        T["credible"].append(t)
        if r < host_reps:
            t0 = time.perf_counter()
            back = be.beliefs_read(slots, mans)
            T["read"].append((time.perf_counter() - t0) * 1e3)
            ref = [cr.credible_numpy(man, p, bw, masks[i], cr.MASS, cr.PROBS, Qs[i]) for i, (p, bw, _) in enumerate(back)]
            T["numpy"].append((time.perf_counter() - t0) * 1e3)
            # the two routes give the same answer (the criteria of tests/credible_cases.py; here: the densities within the bound,
            # and the number of beliefs whose counts agree too -- a count may differ where two densities lie within the bound)
            recs, ld, od, qrecs, first = res
            for i in range(n):
                assert np.all(np.abs(ld[i] - ref[i].logdens) <= 1e-12 * (1 + np.abs(ref[i].logdens))), i
                assert abs(qrecs["logdens"][i] - ref[i].q_logdens[0]) <= 1e-12 * (1 + abs(ref[i].q_logdens[0])), i
            agree = sum(np.array_equal(recs["n_inside"][i, :3], ref[i].n_inside) and qrecs["n_above"][i] == ref[i].q_n_above[0] for i in range(n))
    be.close()
    recs, _, _, qrecs, _ = res
    out += [f"## {n} resident {name} belief{'s' if n > 1 else ''}: N^2 = {N * N} kernel terms twice per belief and {N} twice per query; "
            f"levels, counts and n_above equal to the host's in {agree} of {n} beliefs; mass of the reference point median "
            f"{np.median(qrecs['mass']):.3f}, coverage at 0.5 / 0.9 / 0.95: {cr.coverage(qrecs['mass']).round(3).tolist()}",
            line("device: run_credible (one launch, one copy each way)", T["credible"]),
            line("host route: beliefs_read of the same slots", T["read"]),
            line("host route: beliefs_read + credible_numpy of every belief", T["numpy"])]
    return np.median(T["credible"]), np.median(T["numpy"])


def calibration(V, N, seeds, out):
    truth = {f"x{i}": [float(i), float(i)] for i in range(V)}
    at = (0.5, 0.9, 0.95)
    pooled = []
    out.append(f"## calibration: {V}-pose Euclid(2) chain (one prior at x0, truth x_i = (i, i)), N = {N}, solved in a SolveSession; "
               f"coverage(ses.credibility(truth)) at {at}; nominal coverage = the mass itself")
    for seed in range(1, seeds + 1):
        fg = iif.generateChainEuclid(V, vardims=2, priorEvery=V, N=N)
        with iif.SolveSession(fg) as ses:  # (backend None: libnbp)
            ses.solve(seed=seed)
            t, cred = timed(lambda: ses.credibility(truth))
        m = np.array([cred[f"x{i}"].mass for i in range(V)])
        pooled.append(m)
        out.append(f"seed {seed:2d}: coverage {cr.coverage(m, at).round(3).tolist()}, median mass of the truth {np.median(m):.3f}, "
                   f"ses.credibility of {V} variables {t:.3f} ms")
    P = np.array(pooled)
    out.append(f"pooled over {seeds} seeds x {V} variables: coverage {cr.coverage(P.reshape(-1), at).round(4).tolist()} at nominal {list(at)}")
    for lo in range(0, V, max(V // 5, 1)):
        hi = min(lo + max(V // 5, 1), V)
        out.append(f"  poses x{lo} .. x{hi - 1}: coverage {cr.coverage(P[:, lo:hi].reshape(-1), at).round(3).tolist()}")
    out.append("(the masses of neighbouring poses of one solve are dependent: the chain drifts as a whole, so the pooled figure has far fewer "
               "than seeds x poses independent trials)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--beliefs", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = [f"# nbp_run_credible beside the host route, N = {args.N}, masses {cr.MASS}, probabilities {cr.PROBS}, one reference point per "
           "belief, per-particle outputs included, one MI355X; host clock around each call (the device calls end in a stream "
           "synchronise); median [min, max]; the legs alternate in one process, 3 warm-up rounds first.  Kernel times under rocprofv3 "
           "not taken."]
    print(out[0], flush=True)
    for man, name in ((abi.EUCLID2, "Euclid(2)"), (abi.SE2, "SE(2)")):
        for n in args.beliefs:
            d, h = measure(man, name, n, args.N, args.reps, min(args.host_reps, 1 if n >= 1000 else args.host_reps), out)
            out.append(f"host route / device: {h / d:.1f}")
            print("\n".join(out[-5:]), flush=True)
    k = len(out)
    calibration(args.poses, args.N, args.seeds, out)
    print("\n".join(out[k:]), flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
