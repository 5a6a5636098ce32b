#!/usr/bin/env python3
"""Timings of the scene kernel against the routes that gave the same picture before it existed (DESIGN.md 6,
profiles/scene_grid.txt).  Not a test.

    tools/measure_scene.py [--out profiles/scene_grid.txt] [--repeat 20] [--beliefs 100,1000,10000] [--grids 512,1024]

The driver starts one process per (manifold, number of beliefs) under its own `timeout`, in a chain that stops at the first one that
fails.  A process holds V beliefs of N = 200 points along a boustrophedon chain of unit steps (Euclid(2), or SE(2) drawn on x and y),
bandwidths fitted on the device, and times, each call ending in a synchronise and with the copy back included:

  scene      run_scene_grid on n x n with the automatic extent, reach 6 and inf
  marginals  the route there was: ONE run_marginal_grid of V descriptors on the common extent, V n n doubles copied back, added on
             the host -- where V n n doubles fit in 2.2 GB
  numpy      beliefs_read + scene_grid_numpy (exact=False: numpy's matrix product), reach 6, V <= 1000, three runs
  one        one belief through run_scene_grid against run_marginal_grid on the same grid, alternating; and both on a 2 x 2 grid,
             where a call is its launches and copies and nothing else

Times are host-clock medians (min .. max) over --repeat calls after 2 warm-up calls; a route whose warm-up call takes more than a
second is timed over 5 calls, more than five seconds over 2, and one whose predicted work exceeds --max-pairs (tile, belief) pairs is
not run at all: the row says so."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 200


def _chain(V, D, seed):
    """V clouds of N points, unit steps along a boustrophedon path on a square lattice"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(V)))
    i = np.arange(V)
    row, col = i // side, i % side
    col = np.where(row % 2 == 0, col, side - 1 - col)
    X = np.zeros((V, N, D))
    X[:, :, 0] = col[:, None] + rng.normal(0, 0.1, (V, N))
    X[:, :, 1] = row[:, None] + rng.normal(0, 0.1, (V, N))
    if D == 3:
        X[:, :, 2] = (rng.normal(0, 0.3, (V, N)) + np.pi) % (2 * np.pi) - np.pi
    return X


def _se2_points(X):
    c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
    return np.stack([X[:, 0], X[:, 1], c, s, -s, c], axis=1)


def _timed(fn, repeat):
    t = time.perf_counter()
    fn()
    first = time.perf_counter() - t
    repeat = 2 if first > 5 else 5 if first > 1 else repeat
    if first <= 1:
        fn()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "runs": repeat}


def step(kind, V, grids, repeat, max_pairs):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    abi, sc = iif.abi, iif.scene
    se2 = kind == "se2"
    man = abi.SE2 if se2 else abi.EUCLID2
    D = abi.MANIFOLD_DIM[man]
    X = _chain(V, D, 7)
    be = iif.HipBackend(N, V)
    rows = []
    try:
        slots, mans = list(range(V)), [man] * V
        be.beliefs_write(slots, mans, [((_se2_points(x) if se2 else x), np.full(D, 0.2), None) for x in X])
        be.run_bandwidth(slots, mans)
        for n in grids:
            nn, tiles = (n, n), ((n + 31) // 32) ** 2
            for reach in (6.0, np.inf):
                row = {"route": "scene", "manifold": kind, "V": V, "n": n, "reach": reach, "tiles": tiles}
                if not np.isfinite(reach) and tiles * V > max_pairs:
                    row["not_run"] = f"{tiles * V} (tile, belief) pairs of {N} x 1024 multiply-adds each"
                    rows.append(row)
                    continue
                res = {}

                def run():
                    res["r"] = be.run_scene_grid(slots, mans, (0, 1), nn, None, reach=reach)
                row.update(_timed(run, repeat))
                g, ext, _, skipped, tb = res["r"]
                row.update(tile_beliefs=int(tb), share=tb / (tiles * V), mass=float(g.sum() * ext[1] * ext[3]), extent=ext.tolist())
                rows.append(row)
            ext = rows[-2]["extent"]   # (the reach 6 row: always run)
            if V * n * n * 8 <= 2.2e9:
                req = [(s, man, (0, 1), nn, ext) for s in slots]
                res = {}

                def old():
                    total = np.zeros(nn)
                    for g in be.run_marginal_grid(req):
                        total += g
                    res["g"] = total
                row = {"route": "marginals + host sum", "manifold": kind, "V": V, "n": n, "copied_back_MB": V * n * n * 8 / 1e6}
                row.update(_timed(old, repeat))
                rows.append(row)
            if V <= 1000:
                def host():
                    back = be.beliefs_read(slots, mans)
                    bel = [(man, iif.ppe_coords(man, p), bw, (0, 1)) for p, bw, _ in back]
                    sc.scene_grid_numpy(bel, nn, ext[0::2], ext[1::2], reach=6.0, exact=False)
                row = {"route": "beliefs_read + scene_grid_numpy", "manifold": kind, "V": V, "n": n, "reach": 6.0}
                row.update(_timed(host, 3))
                rows.append(row)
        if V <= 100 and not se2:
            # one belief: the same inner loop as the marginal kernel; what differs is the preparation launch and the record scan
            for n in (grids[0], 2):
                x = X[0]
                e = [x[:, 0].min() - 1.0, (np.ptp(x[:, 0]) + 2.0) / (n - 1), x[:, 1].min() - 1.0, (np.ptp(x[:, 1]) + 2.0) / (n - 1)]
                a = _timed(lambda: be.run_scene_grid([0], [man], (0, 1), (n, n), e, reach=np.inf), repeat)
                b = _timed(lambda: be.run_marginal_grid([(0, man, (0, 1), (n, n), e)]), repeat)
                a = _timed(lambda: be.run_scene_grid([0], [man], (0, 1), (n, n), e, reach=np.inf), repeat)   # (again: after both are warm)
                rows.append({"route": "one belief", "n": n, "scene": a, "marginal": b, "ratio_of_medians": a["median_ms"] / b["median_ms"]})
    finally:
        be.close()
    return rows


def _fmt(r):
    t = f"{r['median_ms']:10.2f} ms ({r['min_ms']:.2f} .. {r['max_ms']:.2f}, {r['runs']} runs)" if "median_ms" in r else f"not run: {r.get('not_run')}"
    if r["route"] == "scene":
        extra = f"  tile_beliefs {r['tile_beliefs']} = {100 * r['share']:.2f} % of {r['tiles']} tiles x V, mass / V {r['mass'] / r['V']:.4f}" if "share" in r else ""
        return f"{r['manifold']:7s} V={r['V']:<6d} n={r['n']:<5d} reach {r['reach']!s:4s} scene                        {t}{extra}"
    if r["route"] == "one belief":
        return (f"one belief, n={r['n']}: run_scene_grid {r['scene']['median_ms']:.3f} ms ({r['scene']['min_ms']:.3f} .. {r['scene']['max_ms']:.3f}), "
                f"run_marginal_grid {r['marginal']['median_ms']:.3f} ms ({r['marginal']['min_ms']:.3f} .. {r['marginal']['max_ms']:.3f}), ratio {r['ratio_of_medians']:.2f}")
    extra = f"  {r['copied_back_MB']:.0f} MB copied back" if "copied_back_MB" in r else ""
    return f"{r['manifold']:7s} V={r['V']:<6d} n={r['n']:<5d} reach {r.get('reach', 'inf')!s:4s} {r['route']:28s} {t}{extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_grid.txt"))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--beliefs", default="100,1000,10000")
    ap.add_argument("--grids", default="512,1024")
    ap.add_argument("--max-pairs", type=int, default=300000)
    ap.add_argument("--limit", type=int, default=240, help="seconds per process")
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    grids = [int(v) for v in args.grids.split(",")]
    if args.step:
        kind, V = args.step.split(":")
        print("RESULT " + json.dumps(step(kind, int(V), grids, args.repeat, args.max_pairs)))
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--repeat", str(args.repeat), "--grids", args.grids, "--max-pairs", str(args.max_pairs)]
    lines = [f"# scene densities: tools/measure_scene.py, N = {N}, bandwidths fitted on the device, host clock around calls that synchronise,",
             "# the copy back included; medians (min .. max)"]
    for kind in ("euclid2", "se2"):
        for V in (int(v) for v in args.beliefs.split(",")):
            p = subprocess.run(["timeout", "-k", "10", str(args.limit)] + me + ["--step", f"{kind}:{V}"], capture_output=True, text=True)
            if p.returncode != 0:  # a fault, an abort or a time limit: nothing more is started
                print(p.stdout[-2000:] + p.stderr[-2000:])
                print(f"step {kind}:{V} ended with status {p.returncode}: stopping")
                open(args.out, "w").write("\n".join(lines + [f"# step {kind}:{V} ended with status {p.returncode}: nothing more was started"]) + "\n")
                return 1
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    for r in json.loads(line[7:]):
                        lines.append(_fmt(r))
                        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
