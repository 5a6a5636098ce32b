#!/usr/bin/env python3
"""Timings of the local products on a grid, and the gap between solved beliefs and their grid products (DESIGN.md 6,
profiles/product_grid.txt).  Not a test.

    tools/measure_productgrid.py [--out profiles/product_grid.txt] [--repeat 20]

The driver starts one process per step under its own `timeout`, in a chain that stops at the first one that fails.  Beliefs hold N =
200 points.  Timed, each call ending in a synchronise and with the copy back included:

  e2       one Euclid(2) pose between two neighbours (two LinearRelative factors) at 64^2, 256^2 and 1024^2 cells
  se2      one SE(2) pose between two neighbours (two ManifoldFactors) at 64 x 64 x 32
  chain:V  every pose of a V-pose Euclid(2) chain (prior on the first, LinearRelative between neighbours) at 64^2, ONE run_product_grid
  numpy    beside each: beliefs_read + product_grid_numpy, at the sizes numpy finishes in about a minute (one to three runs)

Reported and not asserted (the `gaps` steps): after a solve on the device, per variable, the shift of the solved belief's mean from
the mean of its grid product in units of the product's standard deviation (the largest over the coordinates), and the ratio of the
variances (solved / product, first coordinate) -- on the config-2 chain (1000 Euclid(2) poses, a prior every 100) and on the
circular-doors graph.  Grids: 128 cells per axis, 12 bandwidths of margin.

Times are host-clock medians (min .. max) over --repeat calls after 2 warm-up calls; a route whose first call takes more than a second
is timed over 3 calls, more than ten seconds over 1."""
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


def _timed(fn, repeat):
    t = time.perf_counter()
    fn()
    first = time.perf_counter() - t
    repeat = 1 if first > 10 else 3 if first > 1 else repeat
    if first <= 1:
        fn()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "runs": repeat}


def _chain_graph(iif, V, se2=False, seed=7):
    """V poses one unit apart along x, clouds of N points set by hand (sigma 0.1), a prior on the first, relative factors between"""
    rng = np.random.default_rng(seed)
    fg = iif.initfg(iif.SolverParams(N=N))
    for i in range(V):
        if se2:
            iif.addVariable(fg, f"x{i}", iif.SpecialEuclidean2)
            X = np.stack([rng.normal(i, 0.1, N), rng.normal(0, 0.1, N), rng.normal(0, 0.05, N)], axis=1)
            c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
            iif.setValKDE(fg, f"x{i}", np.stack([X[:, 0], X[:, 1], c, s, -s, c], axis=1), [0.05, 0.05, 0.02])
        else:
            iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
            iif.setValKDE(fg, f"x{i}", rng.normal([float(i), 0.0], 0.1, (N, 2)), [0.05, 0.05])
    if not se2:
        iif.addFactor(fg, ["x0"], iif.Prior(iif.MvNormal([0.0, 0.0], [0.1, 0.1])))
    for i in range(V - 1):
        f = iif.ManifoldFactor(iif.MvNormal([1.0, 0.0, 0.0], [0.1, 0.1, 0.05])) if se2 else iif.LinearRelative(iif.MvNormal([1.0, 0.0], [0.1, 0.1]))
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], f)
    return fg


def _resident(iif, fg, labels):
    """the beliefs of the graph in slots of a backend, as a session holds them -> (backend, place)"""
    be = iif.HipBackend(N, len(labels))
    vs = [fg.getVariable(v) for v in labels]
    be.beliefs_write(list(range(len(vs))), [v.varType.manifold for v in vs], [(v.val, v.bw, None) for v in vs])
    return be, {v: i for i, v in enumerate(labels)}


def step_timing(kind, repeat):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    pg = iif.productgrid
    rows = []
    if kind in ("e2", "se2"):
        fg = _chain_graph(iif, 3, se2=kind == "se2")
        targets, sizes = ["x1"], ([[64, 64], [256, 256], [1024, 1024]] if kind == "e2" else [[64, 64, 32]])
        host_cells = 1 << 17
    else:
        V = int(kind.split(":")[1])
        fg = _chain_graph(iif, V)
        targets, sizes = [f"x{i}" for i in range(V)], [[64, 64]]
        host_cells = 100 * 4096
    labels = sorted(fg.ls(), key=pg._natural)
    plans = [pg.variable_items(fg, v) for v in targets]
    be, place = _resident(iif, fg, labels)
    try:
        for n in sizes:
            cells = int(np.prod(n)) * len(targets)
            res = {}

            def dev():
                res["r"] = pg.run_plans(be, plans, place, n)
            row = {"route": "run_product_grid", "what": kind, "n": n, "grids": len(targets), "pair_terms": cells * 2 * N}
            row.update(_timed(dev, repeat))
            r0 = res["r"][targets[0]]
            row.update(logZ=r0.logZ, mass=float(r0.density().sum() * np.prod(r0.extent[1::2])))
            rows.append(row)
            if cells <= host_cells:
                def host():
                    mans = [fg.getVariable(v).varType.manifold for v in labels]
                    back = dict(zip(labels, be.beliefs_read(list(range(len(labels))), mans)))
                    for p in plans:
                        items = [(d, role, None if o is None else back[o][0], g, lp) for d, role, o, g, lp in p.items]
                        pg.product_grid_numpy(p.manifold, n, res["r"][p.label].extent, items)
                row = {"route": "beliefs_read + product_grid_numpy", "what": kind, "n": n, "grids": len(targets)}
                row.update(_timed(host, 3))
                rows.append(row)
            else:
                rows.append({"route": "beliefs_read + product_grid_numpy", "what": kind, "n": n, "grids": len(targets),
                             "not_run": f"{cells * 2 * N:.1e} pair terms on the host"})
    finally:
        be.close()
    return rows


def step_gaps(kind):
    import iif_amd_loader
    iif = iif_amd_loader.load()
    pg = iif.productgrid
    if kind == "chain":
        fg, name = iif.generateChainEuclid(1000, vardims=2, priorEvery=100, N=N), "config-2 chain (1000 Euclid(2) poses, a prior every 100)"
    else:
        fg, name = iif.generateCircularDoors(nposes=100, N=N, sightEvery=10), "circular doors (100 poses, a sighting every 10)"
    rows = []

    def make(n, n_slots, side_ints=0):  # (a session sizes its own context: it takes a factory)
        return iif.HipBackend(n, n_slots, side_ints=side_ints)
    make.is_hip = True
    with iif.SolveSession(fg, backend=make) as ses:
        ses.solve(seed=1)
        grids = ses.localProductGrids(n=128, margin=12.0)
    for v, r in grids.items():
        mean, cov = r.moments()
        var = fg.getVariable(v)
        m, c = iif.meancov_numpy(var.varType.manifold, var.val)
        d = m - mean
        for a, circ in enumerate(iif.ppe._circular(var.varType.manifold)):
            if circ:
                d[a] = (d[a] + np.pi) % (2 * np.pi) - np.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            rows.append({"v": v, "shift": float(np.abs(d / np.sqrt(np.diag(cov))).max()), "ratio": float(c[0, 0] / cov[0, 0]),
                         "factors": len(r.factors), "skipped": len(r.skipped), "logZ": r.logZ})
    return [{"route": "gaps", "what": name, "rows": rows}]


def _fmt(r):
    if r["route"] == "gaps":
        rows = [x for x in r["rows"] if x["factors"] and np.isfinite(x["shift"]) and np.isfinite(x["ratio"])]
        sh, ra = np.array([x["shift"] for x in rows]), np.array([x["ratio"] for x in rows])
        out = [f"# gaps, {r['what']}: solved belief against its grid product, {len(rows)} variables with a supported factor of {len(r['rows'])}",
               f"#   mean shift / sigma_product: median {np.median(sh):.3f}, 90 % {np.quantile(sh, 0.9):.3f}, max {sh.max():.3f} ({rows[int(sh.argmax())]['v']})",
               f"#   variance solved / product:  median {np.median(ra):.3f}, 5 % {np.quantile(ra, 0.05):.3f}, 95 % {np.quantile(ra, 0.95):.3f}, "
               f"min {ra.min():.3f} ({rows[int(ra.argmin())]['v']}), max {ra.max():.3f} ({rows[int(ra.argmax())]['v']})",
               f"#   the ends: {rows[0]['v']} shift {rows[0]['shift']:.3f} ratio {rows[0]['ratio']:.3f}; {rows[-1]['v']} shift {rows[-1]['shift']:.3f} ratio {rows[-1]['ratio']:.3f}",
               "#   per variable: label shift ratio"]
        cells = [f"{x['v']} {x['shift']:.2f} {x['ratio']:.2f}" for x in r["rows"]]
        out += ["  " + "; ".join(cells[k:k + 8]) for k in range(0, len(cells), 8)]
        return "\n".join(out)
    t = f"{r['median_ms']:10.3f} ms ({r['min_ms']:.3f} .. {r['max_ms']:.3f}, {r['runs']} runs)" if "median_ms" in r else f"not run: {r.get('not_run')}"
    extra = f"  {r['pair_terms']:.2e} pair terms, logZ {r['logZ']:.4f}, mass {r['mass']:.6f}" if "pair_terms" in r else ""
    return f"{r['what']:10s} {'x'.join(str(k) for k in r['n']):10s} grids {r['grids']:<5d} {r['route']:34s} {t}{extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "product_grid.txt"))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--steps", default="e2,se2,chain:100,chain:1000,gaps:chain,gaps:doors")
    ap.add_argument("--limit", type=int, default=280, help="seconds per process")
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        rows = step_gaps(args.step.split(":")[1]) if args.step.startswith("gaps:") else step_timing(args.step, args.repeat)
        print("RESULT " + json.dumps(rows))
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--repeat", str(args.repeat)]
    lines = [f"# local products on a grid: tools/measure_productgrid.py, N = {N}, host clock around calls that synchronise, the copy back included;",
             "# medians (min .. max)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for s in args.steps.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(args.limit)] + me + ["--step", s], capture_output=True, text=True)
        if p.returncode != 0:  # a fault, an abort or a time limit: nothing more is started
            print(p.stdout[-2000:] + p.stderr[-2000:])
            print(f"step {s} ended with status {p.returncode}: stopping")
            open(args.out, "w").write("\n".join(lines + [f"# step {s} ended with status {p.returncode}: nothing more was started"]) + "\n")
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                for r in json.loads(line[7:]):
                    lines.append(_fmt(r))
                    print(lines[-1], flush=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
