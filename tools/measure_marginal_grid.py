#!/usr/bin/env python3
"""Timings of the marginal-grid kernel against the routes that gave the same numbers before it existed (DESIGN.md 6,
profiles/marginal_grid_kernel.txt).  Not a test.

    tools/measure_marginal_grid.py [--out DIR] [--beliefs 1000] [--repeat 20]

The driver starts every step as a process of its own under its own `timeout`, in a chain that stops at the first step that fails:

  grid2d   1000 resident Euclid(2) beliefs at N = 200 (bandwidths fitted on the device), 64 x 64 grids with explicit extents:
           nbp_run_marginal_grid against nbp_run_evaluate at the same 4096 points per belief (the upload of the query points is part
           of that route), alternating in one process, every call ending in a synchronise; the two results are compared; also the
           read-back of the beliefs (what the host route pays first)
  grid1d   the same beliefs, 257 points of coordinate 0
  se2xy    1000 SE(2) beliefs, the x-y picture (nbp_run_evaluate cannot give it: nbp_run_evaluate_marginal is the other route)
  host     no device: marginal_grid_numpy of 64 of the Euclid(2) beliefs on 16 processes, scaled to the batch
  trace    rocprofv3 --kernel-trace --stats around a short grid2d, for the kernels' own times (skipped where rocprofv3 is missing)

Times are host-clock medians over --repeat calls after 3 warm-up calls of each route."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 200


def _clouds(manifold_dim, count, seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-5, 5, (count, 1, manifold_dim))
    return centres + rng.normal(0, 0.5, (count, N, manifold_dim))


def _se2_points(X):
    c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
    return np.stack([X[:, 0], X[:, 1], c, s, -s, c], axis=1)


def _median_ms(fn, repeat):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _alternate(a, b, repeat):
    for _ in range(3):
        a()
        b()
    ta, tb = [], []
    for _ in range(repeat):
        t = time.perf_counter()
        a()
        ta.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        b()
        tb.append((time.perf_counter() - t) * 1e3)
    return [float(np.median(ta)), float(np.min(ta)), float(np.max(ta))], [float(np.median(tb)), float(np.min(tb)), float(np.max(tb))]


def device_step(step, B, repeat):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    abi, mg = iif.abi, iif.marginal
    se2 = step == "se2xy"
    man = abi.SE2 if se2 else abi.EUCLID2
    D = abi.MANIFOLD_DIM[man]
    X = _clouds(D, B, 11)
    if se2:
        X[:, :, 2] = (X[:, :, 2] * 0.3 + np.pi) % (2 * np.pi) - np.pi
    be = iif.HipBackend(N, B)
    try:
        slots, mans = list(range(B)), [man] * B
        be.beliefs_write(slots, mans, [((_se2_points(x) if se2 else x), np.full(D, 0.2), None) for x in X])
        be.run_bandwidth(slots, mans)
        t = time.perf_counter()
        back = be.beliefs_read(slots, mans)
        readback_ms = (time.perf_counter() - t) * 1e3
        bws = np.array([bw for _, bw, _ in back])
        dims, n = ((0,), (257,)) if step == "grid1d" else ((0, 1), (64, 64))
        ext = np.zeros((B, 4))
        for a, d in enumerate(dims):
            lo, hi = X[:, :, d].min(axis=1) - 4 * bws[:, d], X[:, :, d].max(axis=1) + 4 * bws[:, d]
            ext[:, 2 * a], ext[:, 2 * a + 1] = lo, (hi - lo) / (n[a] - 1)
        descs = (abi.GridDesc * B)(*[be._grid_desc(s, man, dims, n, ext[s, :2 * len(dims)]) for s in slots])
        pts = int(np.prod(n))
        first = (np.arange(B + 1) * pts).astype(np.int32)
        grid_out, ext_out = np.zeros(B * pts), np.zeros((B, 4))
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        s32, m32 = np.array(slots, dtype=np.int32), np.array(mans, dtype=np.int32)

        def run_grid():
            be._check(be.lib.nbp_run_marginal_grid(be._ctx, descs, B, first.ctypes.data_as(ip), grid_out.ctypes.data_as(dp),
                                                   ext_out.ctypes.data_as(dp)))

        # the other route: the same points as queries, built once on the host (their upload is part of every call)
        Q = np.zeros((B * pts, abi.MAXD))
        for s in slots:
            Q[s * pts:(s + 1) * pts, :D] = _grid_queries(mg, ext[s], n, dims, D)
        eval_out = np.zeros(B * pts)
        masks = np.full(B, sum(1 << d for d in dims), dtype=np.int32)

        def run_eval():
            if se2 or step == "grid1d":
                be._check(be.lib.nbp_run_evaluate_marginal(be._ctx, s32.ctypes.data_as(ip), m32.ctypes.data_as(ip), masks.ctypes.data_as(ip), B,
                                                           first.ctypes.data_as(ip), Q.ctypes.data_as(dp), eval_out.ctypes.data_as(dp)))
            else:
                be._check(be.lib.nbp_run_evaluate(be._ctx, s32.ctypes.data_as(ip), m32.ctypes.data_as(ip), B, first.ctypes.data_as(ip),
                                                  Q.ctypes.data_as(dp), eval_out.ctypes.data_as(dp)))

        tg, te = _alternate(run_grid, run_eval, repeat)
        rel = float(np.max(np.abs(grid_out - eval_out) / np.maximum(eval_out, 1e-280)))
        return {"step": step, "beliefs": B, "N": N, "manifold": int(man), "dims": list(dims), "n": list(n),
                "grid_kernel_route_ms": tg, "evaluate_route": "nbp_run_evaluate_marginal" if (se2 or step == "grid1d") else "nbp_run_evaluate",
                "evaluate_route_ms": te, "ratio_of_medians": te[0] / tg[0], "max_relative_difference": rel,
                "beliefs_readback_ms": readback_ms, "timing": "host clock around calls that synchronise: median, min, max"}
    finally:
        be.close()


def _grid_queries(mg, ext, n, dims, D):
    axes = mg.grid_axes(ext, n)
    mesh = np.meshgrid(*axes, indexing="ij")
    q = np.zeros((mesh[0].size, D))
    for a, d in enumerate(dims):
        q[:, d] = mesh[a].reshape(-1)
    return q


def _host_one(x):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    return iif.marginal.marginal_grid_numpy(iif.abi.EUCLID2, x, [0.2, 0.2], (0, 1), (64, 64))[0].sum()


def host_step(B):
    from concurrent.futures import ProcessPoolExecutor
    X = _clouds(2, 64, 11)
    with ProcessPoolExecutor(16) as ex:
        list(ex.map(_host_one, X[:16]))  # start the workers
        t = time.perf_counter()
        list(ex.map(_host_one, X))
        dt = time.perf_counter() - t
    return {"step": "host", "beliefs_timed": 64, "processes": 16, "seconds": dt, "scaled_to_beliefs": B, "scaled_ms": dt / 64 * B * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "marginal_grid_out"))
    ap.add_argument("--beliefs", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        res = host_step(args.beliefs) if args.step == "host" else device_step(args.step, args.beliefs, args.repeat)
        print("RESULT " + json.dumps(res))
        return 0
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--beliefs", str(args.beliefs)]
    steps = [("grid2d", 240, me + ["--step", "grid2d", "--repeat", str(args.repeat)]),
             ("grid1d", 180, me + ["--step", "grid1d", "--repeat", str(args.repeat)]),
             ("se2xy", 240, me + ["--step", "se2xy", "--repeat", str(args.repeat)]),
             ("host", 240, me + ["--step", "host"])]
    if shutil.which("rocprofv3"):
        steps.append(("trace", 300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(args.out, "trace"), "--"] + me +
                      ["--step", "grid2d", "--repeat", "3"]))
    results = []
    for name, limit, cmd in steps:
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        open(os.path.join(args.out, name + ".log"), "w").write(p.stdout + p.stderr)
        if p.returncode != 0:  # a fault, an abort or a time limit: nothing more is started
            print(f"step {name} ended with status {p.returncode}: stopping (see {name}.log)")
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("RESULT ") and name != "trace":
                results.append(json.loads(line[7:]))
                print(line[7:])
    for dp_, _, fs in os.walk(os.path.join(args.out, "trace")):
        for f in fs:
            if f.endswith("kernel_stats.csv"):
                for line in open(os.path.join(dp_, f)):
                    if "Name" in line or "marginal" in line or "nbp_eval_kernel" in line:
                        print("trace: " + line.strip())
    json.dump(results, open(os.path.join(args.out, "results.json"), "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
