"""Cases shared by the two legs of the local-product-on-a-grid tests (test_productgrid.py on the host, test_gpu_productgrid.py on the
device): the items -- every measurement model of likelihood_cases' table in every role the planner admits --, the grids they are
asked on, and the device-against-restatement tolerance, worked out per cell from the restatement's own rounding noise by the rule
likelihood_cases.restate uses: 16 max(|float64 - long double|, 4 ulp(max(1, |l|)))."""
import numpy as np

import likelihood_cases as lc
from parity_utils import abi, iif

pg = iif.productgrid
lik = iif.likelihood

# (case of likelihood_cases.CASES, role of the grid's variable): a prior has role 0 alone
ITEM_CASES = [(name, role) for name in lc.CASES for role in ((0,) if lc.unary(name) else (0, 1))]
MANIFOLDS = (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3, abi.CIRCULAR, abi.SE2)


def by_manifold(m):
    return [(name, role) for name, role in ITEM_CASES if lc.CASES[name][1] == m]


def extent_for(manifold, n, lo=-3.0, hi=3.5):
    """an explicit extent over the clouds of likelihood_cases.clouds: Euclidean axes lo .. hi, circular axes the whole circle"""
    circ = iif.ppe._circular(manifold)
    ext = []
    for a, c in enumerate(circ):
        ext += [-np.pi, 2 * np.pi / n[a]] if c else [lo, (hi - lo) / max(n[a] - 1, 1)]
    return np.array(ext)


def cloud(manifold, n, rng, centre=0.8):
    """host points (n x P) of a neighbour: several units wide, headings and angles over the whole circle"""
    import ppe_cases as pc
    D = abi.MANIFOLD_DIM[manifold]
    X = rng.normal(centre, 1.5, (n, D))
    for d in pc.circular_coords(manifold):
        X[:, d] = rng.uniform(-np.pi, np.pi, n)
    return pc.to_points(manifold, X)


def items_for(cases, counts, rng, groups=None, log_priors=None):
    """[(desc, role, other host points or None, group, log_prior)] for `cases` = [(name, role)]: item k's other cloud has counts[k]
    points; groups default to one per item with log_prior 0"""
    out = []
    for k, (name, role) in enumerate(cases):
        m = lc.CASES[name][1]
        other = None if lc.unary(name) else cloud(m, counts[k], rng)
        out.append((lc.desc(name), role, other, k if groups is None else groups[k], 0.0 if log_priors is None else log_priors[k]))
    return out


def _tol(a64, a80):
    a, b = np.asarray(a64, dtype=np.float64), np.asarray(a80, dtype=np.longdouble)
    with np.errstate(invalid="ignore"):
        noise = np.abs((a.astype(np.longdouble) - b).astype(np.float64))
        ulp = 4 * np.spacing(np.maximum(1.0, np.abs(a)))
    fin = np.isfinite(a)
    return np.where(fin, 16 * np.maximum(np.where(fin, noise, 0.0), np.where(fin, ulp, 0.0)), 0.0)


def restate(manifold, n, extent, items):
    """the restatement of one grid in float64 and in long double -> (logp, logZ, logmax, argmax, tol_logp, tol_logZ): computed on the
    host, never from the device"""
    l64, z64, m64, a64 = pg.product_grid_numpy(manifold, n, extent, items)
    l80, z80, _, _ = pg.product_grid_numpy(manifold, n, extent, items, dtype=np.longdouble)
    return np.asarray(l64, dtype=np.float64), float(z64), float(m64), a64, _tol(l64, l80), float(_tol(z64, z80))


def hold(logp, rec, ref, what):
    """a device grid (values, (logZ, logmax, argmax)) against `restate`: finite cells within the tolerance, -inf cells and argmax
    exactly.  Prints the largest error / tolerance before it asserts; returns it"""
    l64, z64, m64, a64, tl, tz = ref
    logp = np.asarray(logp)
    assert logp.shape == l64.shape, (what, logp.shape, l64.shape)
    fin = np.isfinite(l64)
    assert np.array_equal(logp[~fin], l64[~fin]), f"{what}: the cells outside every support differ"
    with np.errstate(invalid="ignore"):
        ratio = np.abs(logp[fin] - l64[fin]) / tl[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    zr = abs(rec[0] - z64) / tz if np.isfinite(z64) else (0.0 if rec[0] == z64 else np.inf)
    print(f"{what}: cells {worst:.3f} of the tolerance, logZ device {rec[0]!r} restatement {z64!r} ratio {zr:.3f}, argmax {rec[2]} / {a64}")
    assert np.all(np.isfinite(logp[fin])) and worst <= 1.0, f"{what}: a cell is {worst:.3f} of its tolerance off"
    assert zr <= 1.0, f"{what}: logZ device {rec[0]!r}, restatement {z64!r}, tolerance {tz:.3e}"
    assert int(rec[2]) == a64, f"{what}: argmax device {rec[2]}, restatement {a64}"
    assert rec[1] == logp.reshape(-1)[rec[2]] if a64 >= 0 else rec[1] == -np.inf, f"{what}: logmax is not the value at argmax"
    return max(worst, zr)
