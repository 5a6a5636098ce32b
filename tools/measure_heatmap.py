#!/usr/bin/env python3
"""Timings of the heatmap density on the device against the only route there was before it: `heatmap_density_numpy` on the host
plus the upload of the points (profiles/heatmap_density.txt).  Not a test.

    tools/measure_heatmap.py [--out DIR] [--repeat 20]

The driver starts every step as a process of its own under its own `timeout`, in a chain that stops at the first step that fails:

  g1000    a 1000 x 1000 field: nbp_heatmap_create, then for M = 10^4 and 10^5 nbp_heatmap_build (no host outputs) and
           nbp_heatmap_draw of N = 512 points into a slot (no host outputs); against heatmap_density_numpy with the same M and
           n = 512 and nbp_belief_write of its points.  Every device call ends in a synchronise.  The two routes' points are compared.
  g4000    the same on 4000 x 4000 cells (128 MB of field)
  trace    rocprofv3 --kernel-trace --stats around a short g4000, for the kernels' own times (skipped where rocprofv3 is missing):
           the two passes of the cell sum read the field twice and write cdf once, 3 x 8 bytes a cell

Times are host-clock medians (min, max) over --repeat calls after 3 warm-up calls; the host route over 3 calls after one."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 512


def _times(fn, repeat, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def device_step(size, repeat, host=True):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    abi, hm = iif.abi, iif.heatmap
    rng = np.random.default_rng(size)
    x = np.linspace(0.0, 10.0 * (size - 1), size)
    data = rng.uniform(0.0, 3.0, (size, size)) + 0.5 * np.sin(x / 500.0)[:, None]
    be = iif.HipBackend(N, 2)
    res = {"step": f"g{size}", "cells": size * size, "n": N, "timing": "host clock around calls that synchronise: median, min, max (ms)"}
    try:
        handles = []

        def create():
            handles.append(be.heatmap_create(data, x, x))
            if len(handles) > 1:
                be.heatmap_destroy(handles.pop(0))
        res["create_ms"] = _times(create, repeat)
        res["create_GB_per_s_if_3x8_bytes_per_cell"] = 24.0 * size * size / (res["create_ms"][0] * 1e6)
        h = handles[0]
        for M in (10_000, 100_000):
            res[f"build_M{M}_ms"] = _times(lambda: be.heatmap_build(h, M, 1, outputs=False), repeat)
            res[f"draw_M{M}_ms"] = _times(lambda: be.heatmap_draw(h, N, 2, slot=1, outputs=False), repeat)
            dev = be.belief_read(1, abi.EUCLID2)[0]
            if host:
                R = {}

                def numpy_route():
                    R.update(hm.heatmap_density_numpy(data, x, x, M=M, n=N, seed=1, seed2=2))
                    be.belief_write(0, abi.EUCLID2, R["points"], R["bw"])
                res[f"host_M{M}_ms"] = _times(numpy_route, 3, warm=1)
                res[f"upload_M{M}_ms"] = _times(lambda: be.belief_write(0, abi.EUCLID2, R["points"], R["bw"]), repeat)
                dev_ms = res["create_ms"][0] + res[f"build_M{M}_ms"][0] + res[f"draw_M{M}_ms"][0]
                res[f"ratio_M{M}_host_over_device_create_build_draw"] = res[f"host_M{M}_ms"][0] / dev_ms
                res[f"ratio_M{M}_host_over_device_build_draw"] = res[f"host_M{M}_ms"][0] / (dev_ms - res["create_ms"][0])
                res[f"max_abs_point_difference_M{M}"] = float(np.max(np.abs(dev - R["points"])))
                res[f"picks_equal_M{M}"] = bool(np.array_equal(be.heatmap_draw(h, N, 2)[0], R["pick"]))
        be.heatmap_destroy(h)
        return res
    finally:
        be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "heatmap_out"))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(device_step(int(args.step[1:]), args.repeat, host=not args.no_host)))
        return 0
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [("g1000", 240, me + ["--step", "g1000", "--repeat", str(args.repeat)]),
             ("g4000", 400, me + ["--step", "g4000", "--repeat", str(args.repeat)])]
    if shutil.which("rocprofv3"):
        steps.append(("trace", 300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(args.out, "trace"), "--"] + me +
                      ["--step", "g4000", "--repeat", "3", "--no-host"]))
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
                print(json.dumps(results[-1], indent=1))
    for dp_, _, fs in os.walk(os.path.join(args.out, "trace")):
        for f in fs:
            if f.endswith("kernel_stats.csv"):
                for line in open(os.path.join(dp_, f)):
                    if "Name" in line or "nbp_hm_" in line:
                        print("trace: " + line.strip())
    json.dump(results, open(os.path.join(args.out, "results.json"), "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
