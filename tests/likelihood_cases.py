"""Cases shared by the two legs of the factor-likelihood tests (test_factor_likelihood.py on the host, test_gpu_factor_likelihood.py
on the device): the table of measurement models -- every kind x every admissible family x its manifolds, full L in two and three
dimensions, partial masks, mixtures of 1 / 2 / 4 components, unary items --, the clouds they are asked about, and the
device-against-restatement tolerance, which is worked out per case from the restatement's own rounding noise."""
import numpy as np

import ppe_cases as pc
from parity_utils import abi, iif

lik = iif.likelihood
G, U, R = abi.DIST_GAUSSIAN, abi.DIST_UNIFORM, abi.DIST_RAYLEIGH

L2 = [[0.6, 0.0], [0.25, 0.4]]
L3 = [[0.5, 0.0, 0.0], [0.2, 0.7, 0.0], [-0.1, 0.15, 0.3]]

# name -> (kind, manifold, components [(weight, mean, L, family)], partial mask)
CASES = {
    # priors (unary)
    "prior_e1_normal": (abi.F_PRIOR, abi.EUCLID1, [(1.0, [0.4], [[0.8]], G)], 0),
    "prior_e1_uniform": (abi.F_PRIOR, abi.EUCLID1, [(1.0, [-1.0], [[3.0]], U)], 0),
    "prior_e1_rayleigh": (abi.F_PRIOR, abi.EUCLID1, [(1.0, [0.0], [[1.2]], R)], 0),
    "prior_e2_full": (abi.F_PRIOR, abi.EUCLID2, [(1.0, [0.2, -0.3], L2, G)], 0),
    "prior_e3_full": (abi.F_PRIOR, abi.EUCLID3, [(1.0, [0.2, -0.3, 0.5], L3, G)], 0),
    "prior_circ_normal": (abi.F_PRIOR, abi.CIRCULAR, [(1.0, [3.0], [[0.5]], G)], 0),
    "prior_se2_full": (abi.F_PRIOR, abi.SE2, [(1.0, [0.2, -0.3, 3.0], L3, G)], 0),
    "prior_se2_xy": (abi.F_PRIOR, abi.SE2, [(1.0, [0.2, -0.3], L2, G)], 3),
    "prior_se2_heading": (abi.F_PRIOR, abi.SE2, [(1.0, [-3.0], [[0.4]], G)], 4),
    "prior_e3_coords13": (abi.F_PRIOR, abi.EUCLID3, [(1.0, [0.2, 0.5], L2, G)], 5),
    "prior_e2_mix2": (abi.F_PRIOR, abi.EUCLID2, [(0.3, [0.2, -0.3], L2, G), (0.7, [-1.0, 1.0], [[0.3, 0.0], [0.0, 0.9]], G)], 0),
    # LinearRelative
    "linrel_e1_normal": (abi.F_LINREL, abi.EUCLID1, [(1.0, [1.0], [[0.7]], G)], 0),
    "linrel_e1_uniform": (abi.F_LINREL, abi.EUCLID1, [(1.0, [-0.5], [[2.5]], U)], 0),
    "linrel_e1_rayleigh": (abi.F_LINREL, abi.EUCLID1, [(1.0, [0.0], [[1.5]], R)], 0),
    "linrel_e2_full": (abi.F_LINREL, abi.EUCLID2, [(1.0, [1.0, 0.5], L2, G)], 0),
    "linrel_e3_full": (abi.F_LINREL, abi.EUCLID3, [(1.0, [1.0, 0.5, -0.5], L3, G)], 0),
    "linrel_e3_coord2": (abi.F_LINREL, abi.EUCLID3, [(1.0, [0.5], [[0.6]], G)], 2),
    "linrel_e3_coords13": (abi.F_LINREL, abi.EUCLID3, [(1.0, [1.0, -0.5], L2, G)], 5),
    "linrel_e2_coord2_uniform": (abi.F_LINREL, abi.EUCLID2, [(1.0, [-1.0], [[3.0]], U)], 2),
    "linrel_e1_mix1": (abi.F_LINREL, abi.EUCLID1, [(2.0, [1.0], [[0.7]], G)], 0),
    "linrel_e1_mix2": (abi.F_LINREL, abi.EUCLID1, [(0.5, [1.0], [[0.7]], G), (0.5, [-2.0], [[0.3]], G)], 0),
    "linrel_e1_mix4": (abi.F_LINREL, abi.EUCLID1, [(0.4, [1.0], [[0.7]], G), (0.3, [-0.5], [[2.5]], U), (0.2, [0.0], [[1.5]], R),
                                                   (0.1, [4.0], [[0.2]], G)], 0),
    # CircularCircular
    "circ_normal": (abi.F_CIRCULAR, abi.CIRCULAR, [(1.0, [3.0], [[0.4]], G)], 0),
    "circ_uniform": (abi.F_CIRCULAR, abi.CIRCULAR, [(1.0, [-1.0], [[2.0]], U)], 0),
    "circ_rayleigh": (abi.F_CIRCULAR, abi.CIRCULAR, [(1.0, [0.0], [[1.0]], R)], 0),
    "circ_mix2": (abi.F_CIRCULAR, abi.CIRCULAR, [(0.6, [3.0], [[0.4]], G), (0.4, [-1.5], [[0.2]], G)], 0),
    # ManifoldFactor on SE(2)
    "se2_full": (abi.F_SE2, abi.SE2, [(1.0, [1.0, 0.5, 3.0], L3, G)], 0),
    "se2_xy": (abi.F_SE2, abi.SE2, [(1.0, [1.0, 0.5], L2, G)], 3),
    "se2_heading": (abi.F_SE2, abi.SE2, [(1.0, [-3.0], [[0.3]], G)], 4),
    "se2_x_uniform": (abi.F_SE2, abi.SE2, [(1.0, [-2.0], [[4.0]], U)], 1),
    "se2_mix4": (abi.F_SE2, abi.SE2, [(0.25, [1.0, 0.5, 3.0], L3, G), (0.25, [-1.0, 0.0, 0.0], L3, G), (0.4, [0.0, 2.0, -1.5], L3, G),
                                      (0.1, [0.0, 0.0, 1.0], [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], G)], 0),
    # EuclidDistance
    "dist_e1_normal": (abi.F_EUCLIDDIST, abi.EUCLID1, [(1.0, [1.5], [[0.5]], G)], 0),
    "dist_e2_normal": (abi.F_EUCLIDDIST, abi.EUCLID2, [(1.0, [2.0], [[0.5]], G)], 0),
    "dist_e3_normal": (abi.F_EUCLIDDIST, abi.EUCLID3, [(1.0, [2.5], [[0.5]], G)], 0),
    "dist_e2_uniform": (abi.F_EUCLIDDIST, abi.EUCLID2, [(1.0, [0.5], [[2.0]], U)], 0),
    "dist_e2_rayleigh": (abi.F_EUCLIDDIST, abi.EUCLID2, [(1.0, [0.0], [[1.5]], R)], 0),
}


def desc(name, slot_a=0, slot_b=-1):
    kind, manifold, comps, mask = CASES[name]
    return lik.likelihood_desc(kind, manifold, comps, mask, slot_a, slot_b)


def unary(name):
    return CASES[name][0] == abi.F_PRIOR


def clouds(name, na, nb, rng):
    """the tangent coordinates of the two roles (b None for a prior): clouds several units wide, headings and angles over the
    whole circle"""
    m = CASES[name][1]
    D = abi.MANIFOLD_DIM[m]

    def one(n, centre):
        X = rng.normal(centre, 1.5, (n, D))
        for d in pc.circular_coords(m):
            X[:, d] = rng.uniform(-np.pi, np.pi, n)
        return X
    return one(na, 0.0), (None if unary(name) else one(nb, 0.8))


def points(name, X):
    return None if X is None else pc.to_points(CASES[name][1], X)


def restate(d, A, B):
    """the restatement of one item in float64 and in long double, and the tolerance a device value is held to:
    16 max(|float64 - long double|, 4 ulp(max(1, |l|))) for loglik and for every comp_loglik -- the restatement's own rounding noise
    measures the case's conditioning; the factor 16 covers the device's own exp / sincos (1 - 1.5 ulp of libm), another block-sum
    tree and up to 512^2 terms.  Computed on the host, never from the device.  -> (loglik, comp_loglik[4], tol, tol_comp[4])"""
    l64, c64 = lik.factor_likelihood_numpy(d, A, B)
    l80, c80 = lik.factor_likelihood_numpy(d, A, B, dtype=np.longdouble)

    def tol(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.longdouble)
        with np.errstate(invalid="ignore"):
            noise = np.abs((a.astype(np.longdouble) - b).astype(np.float64))
            ulp = 4 * np.spacing(np.maximum(1.0, np.abs(a)))
        fin = np.isfinite(a)
        return np.where(fin, 16 * np.maximum(np.where(fin, noise, 0.0), np.where(fin, ulp, 0.0)), 0.0)
    return float(l64), np.asarray(c64, dtype=np.float64), float(tol(l64, l80)), tol(c64, c80)


def hold(got_ll, got_cl, ref, what):
    """a device value against `restate`: finite values within the tolerance, -inf and NaN where the restatement has them.  Prints
    the ratio error / tolerance before it asserts; returns the largest"""
    l64, c64, tl, tc = ref
    worst = 0.0
    for g, r, t, w in [(got_ll, l64, tl, "loglik")] + [(got_cl[k], c64[k], tc[k], f"comp_loglik[{k}]") for k in range(abi.MAXC)]:
        if np.isfinite(r):
            ratio = abs(g - r) / t if np.isfinite(g) else np.inf
            worst = max(worst, ratio)
            print(f"{what} {w}: device {g!r} restatement {r!r} tol {t:.3e} ratio {ratio:.3f}")
            assert ratio <= 1.0, f"{what} {w}: device {g!r}, restatement {r!r}, tolerance {t:.3e}"
        else:
            assert (np.isnan(g) and np.isnan(r)) or g == r, f"{what} {w}: device {g!r}, restatement {r!r}"
    return worst


# ---- the scenes of the weight tests ------------------------------------------------------------------------------------------------
def doors_graph(order=("x", "l1", "l2"), multihypo=None, n=200, seed=7):
    """x ~ N(2.05, 0.1), l1 ~ N(0, 0.1), l2 ~ N(2, 0.1), LinearRelative Normal(0, 0.2) with the landmarks as two hypotheses"""
    rng = np.random.default_rng(seed)
    vals = {"x": rng.normal(2.05, 0.1, (n, 1)), "l1": rng.normal(0.0, 0.1, (n, 1)), "l2": rng.normal(2.0, 0.1, (n, 1))}
    fg = iif.initfg(iif.SolverParams(N=n))
    for v in ("x", "l1", "l2"):
        iif.addVariable(fg, v, iif.ContinuousScalar)
        iif.setValKDE(fg, v, vals[v], [0.05])
    if multihypo is None:
        multihypo = [1.0 if v == "x" else 0.5 for v in order]
    iif.addFactor(fg, list(order), iif.LinearRelative(iif.Normal(0.0, 0.2)), multihypo=multihypo, label="door")
    return fg


def outlier_chain(fg, n_poses=6, n=200, seed=11, off=3):
    """a chain p0 .. p5 on Euclid(2) set by hand one unit apart (sigma 0.1), LinearRelative MvNormal((1, 0), 0.1) between
    neighbours; the factor behind pose `off` expects (6, 0): 50 sigma off"""
    rng = np.random.default_rng(seed)
    for i in range(n_poses):
        iif.addVariable(fg, f"p{i}", iif.ContinuousEuclid(2))
        iif.setValKDE(fg, f"p{i}", rng.normal([float(i), 0.0], 0.1, (n, 2)), [0.05, 0.05])
    iif.addFactor(fg, ["p0"], iif.Prior(iif.MvNormal([0.0, 0.0], [0.1, 0.1])), label="p0f1")
    for i in range(n_poses - 1):
        mu = [6.0, 0.0] if i == off else [1.0, 0.0]
        iif.addFactor(fg, [f"p{i}", f"p{i + 1}"], iif.LinearRelative(iif.MvNormal(mu, [0.1, 0.1])), label=f"p{i}p{i + 1}f1")
    return f"p{off}p{off + 1}f1"
