"""Shared cases of the mixture-summary tests (tests/test_mixture.py on the CPU, tests/test_gpu_mixture.py on the device): the clouds,
the restatement helpers and the tolerances a device result is held to.

The definition is DESIGN.md 3 ("Mixture summaries") / incrementalinference.jl_amd/mixture.py.

Clouds.  The table clouds of modes_cases.py (through `modes_cases.make`) serve the definition's own tests.  The device parity tests
need fits that take many iterations, so they use `blobs`: K Gaussian clusters of sigma 0.3 whose centres lie 0.78 apart along
coordinate 0 (2.6 sigma: neighbours overlap), one particle in ten labelled -1, the starting means a tenth of a sigma off the
centres.  `starved`: a component that starts on one particle in a gap of another's cloud, which the second M-step drops.  `far_pair`: two points 100 apart, one component each (responsibilities exactly 0 and 1).

Device against `mixture_numpy` on the slot as read back (check_device):

  weights, means, covariances, J   within 16 max(|float64 - long double restatement|, 4 ulp(max(1, |v|))) of the float64
                                   restatement: likelihood_cases.restate's recipe, on the same grounds (the device's own exp and
                                   log, another rounding of the same reduction tree).  Computed on the host per case, never from the
                                   device.
  n_comp, n_dropped                equal
  iters                            equal in a tol = 0 run (= max_iter, converged 0); within +-1 in a converged run
  labels, count                    equal, except for particles whose two greatest restated responsibilities differ by less than
                                   1e-6 (at most 1 % of a belief's particles: asserted of the restatement alone, `input_conditions`)

`input_conditions` also asserts that no drop decision sits on the threshold: the least n_k a live component ever had is >= 1, and
the greatest n_k a component was dropped at is < 0.25.
"""
import numpy as np

import modes_cases as mc
import ppe_cases as pc
from parity_utils import abi, iif

mixture = iif.mixture
MANIFOLDS = pc.MANIFOLDS
SIZES = mc.SIZES
MIX_MAX = abi.MIX_MAX
ITERS = (1, 2, 10, 50)
SIGMA, SPACING = 0.3, 0.78
GAP = 1e-6


def bandwidth(manifold):
    return 0.5 * pc.hand_bandwidth(manifold)


def centres(manifold, K):
    """K x D: 0.78 apart along coordinate 0 (from -pi + 0.4 on: eight of them go once round a circle), a fixed wobble elsewhere"""
    D = abi.MANIFOLD_DIM[manifold]
    C = np.zeros((K, D))
    C[:, 0] = -np.pi + 0.4 + SPACING * np.arange(K)
    for d in range(1, D):
        C[:, d] = 0.5 * np.sin((d + 1.0) * np.arange(K) + d)
    for d in pc.circular_coords(manifold):
        C[:, d] = pc.wrap(C[:, d])
    return C


def blobs(manifold, c, K, rng):
    """-> (X tangent coordinates c x D, bandwidth, labels c, init_mean 8 x 3): K = min(K, c) clusters, every one with a labelled
    particle"""
    D = abi.MANIFOLD_DIM[manifold]
    K = min(K, c)
    C = centres(manifold, K)
    which = rng.integers(0, K, size=c)
    which[:K] = np.arange(K)
    X = C[which] + rng.normal(0.0, SIGMA, (c, D))
    for d in pc.circular_coords(manifold):
        X[:, d] = pc.wrap(X[:, d])
    lab = which.astype(np.int32)
    off = rng.uniform(size=c) < 0.1
    off[:K] = False
    lab[off] = -1
    mu = np.zeros((MIX_MAX, abi.MAXD))
    mu[:K, :D] = C + rng.normal(0.0, 0.1 * SIGMA, (K, D))
    for d in pc.circular_coords(manifold):
        mu[:K, d] = pc.wrap(mu[:K, d])
    return np.ascontiguousarray(X), bandwidth(manifold), lab, mu


def starved(manifold, c, rng):
    """a component that the second M-step drops, far from the threshold on both sides.  Component 0 holds two tight clusters
    (sigma 0.1 at -0.6 and +0.6 in coordinate 0), component 1 a blob at 2; component 2 starts on ONE particle at the origin, in the
    gap: n = 1 at the first M-step, and after the first E-step only its own particle answers to it (a few hundredths)"""
    D = abi.MANIFOLD_DIM[manifold]
    which = rng.integers(0, 3, size=c)
    which[:3] = (0, 1, 2)
    cen = np.zeros((3, D))
    cen[:, 0] = (-0.6, 0.6, 2.0)
    X = cen[which] + rng.normal(0.0, 0.1, (c, D)) * np.where(which == 2, 3.0, 1.0)[:, None]
    lab = np.where(which == 2, 1, 0).astype(np.int32)
    X[3], lab[3] = 0.0, 2
    mu = np.zeros((MIX_MAX, abi.MAXD))
    mu[1, 0] = 2.0
    return np.ascontiguousarray(X), bandwidth(manifold), lab, mu


def far_pair(manifold):
    """two points 100 apart in coordinate 0 (on a circle: 3 apart), one component each"""
    D = abi.MANIFOLD_DIM[manifold]
    X = np.zeros((2, D))
    X[1, 0] = 3.0 if manifold == abi.CIRCULAR else 100.0
    X[:, 1:] = 0.25
    mu = np.zeros((MIX_MAX, abi.MAXD))
    mu[:2, :D] = X
    return X, bandwidth(manifold), np.array([0, 1], dtype=np.int32), mu


def tolerance(a64, a80, wrapped=()):
    """16 max(|float64 - long double|, 4 ulp(max(1, |a|))), elementwise (likelihood_cases.restate's recipe); wrapped: the trailing
    coordinates whose difference is taken on the circle (two means on either side of +-pi are close)"""
    a, b = np.asarray(a64, dtype=np.float64), np.asarray(a80, dtype=np.longdouble)
    with np.errstate(invalid="ignore"):
        noise = np.abs((a.astype(np.longdouble) - b).astype(np.float64))
        for k in wrapped:
            noise[..., k] = np.abs(pc.wrap(noise[..., k]))
        ulp = 4 * np.spacing(np.maximum(1.0, np.abs(a)))
    fin = np.isfinite(a)
    return np.where(fin, 16 * np.maximum(np.where(fin, noise, 0.0), np.where(fin, ulp, 0.0)), 0.0)


def restate(manifold, X, bw, lab, mu, tol=abi.MIX_TOL, max_iter=abi.MIX_MAX_ITER, at=None):
    """the restatement in float64 and in long double -> (f64, f80), each a MixtureFit or, with `at`, {t: MixtureFit}"""
    f64 = mixture.mixture_numpy(manifold, X, bw, lab, mu, tol, max_iter, at=at)
    f80 = mixture.mixture_numpy(manifold, X, bw, lab, mu, tol, max_iter, dtype=np.longdouble, at=at)
    return f64, f80


def close_calls(fit):
    """the particles whose two greatest restated responsibilities (among the live components) differ by less than GAP"""
    r = np.sort(np.asarray(fit.resp, dtype=np.float64)[:, fit.rank >= 0], axis=1)
    if r.shape[1] < 2:
        return np.zeros(r.shape[0], dtype=bool)
    return r[:, -1] - r[:, -2] < GAP


def input_conditions(fit, what=""):
    """what a parity case must satisfy on the host, before any device value is looked at"""
    c = len(fit.labels)
    close = int(close_calls(fit).sum())
    assert close <= 0.01 * c, (what, "close calls", close, c)
    assert fit.n_live_min >= 1.0, (what, "a live component fell below one particle", fit.n_live_min)
    assert fit.n_drop_max < 0.25, (what, "a component was dropped near the threshold", fit.n_drop_max)


def coord_diff(manifold, a, b):
    d = np.array(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    for k in pc.circular_coords(manifold):
        d[..., k] = pc.wrap(d[..., k])
    return d


def check_device(manifold, rec, labels_out, f64, f80, what="", converged_run=False):
    """one belief's record and label row of `run_mixture` against the restatement (the criteria of the module docstring) ->
    the greatest error in units of its tolerance"""
    c, K = len(f64.labels), f64.n_comp
    input_conditions(f64, what)
    assert int(rec["n_comp"]) == K and int(rec["n_dropped"]) == f64.n_dropped, (what, rec["n_comp"], K, rec["n_dropped"], f64.n_dropped)
    if converged_run:
        assert int(rec["converged"]) == 1 == f64.converged and abs(int(rec["iters"]) - f64.iters) <= 1, (what, rec["iters"], f64.iters)
    else:
        assert int(rec["iters"]) == f64.iters and int(rec["converged"]) == f64.converged, (what, rec["iters"], f64.iters, rec["converged"])
    worst = 0.0
    for name, dev, a, b in (("weight", rec["weight"], f64.weight, f80.weight), ("cov", rec["cov"], f64.cov, f80.cov),
                            ("objective", rec["objective"], f64.objective, f80.objective)):
        err, tol = np.abs(np.asarray(dev) - np.asarray(a, dtype=np.float64)), tolerance(a, b)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (what, name, float(np.max(err / tol)), dev, a)
    err = np.abs(coord_diff(manifold, rec["mean"], f64.mean))
    tol = tolerance(f64.mean, f80.mean, pc.circular_coords(manifold))
    worst = max(worst, float(np.max(err / tol)))
    assert np.all(err <= tol), (what, "mean", float(np.max(err / tol)), rec["mean"], f64.mean)
    # entries from n_comp on are zero
    assert np.all(rec["weight"][K:] == 0) and np.all(rec["mean"][K:] == 0) and np.all(rec["cov"][K:] == 0) and np.all(rec["count"][K:] == 0)
    D = abi.MANIFOLD_DIM[manifold]
    assert np.all(rec["mean"][:, D:] == 0) and np.all(rec["cov"][:, D:, :] == 0) and np.all(rec["cov"][:, :, D:] == 0), what
    assert np.array_equal(rec["cov"], np.swapaxes(rec["cov"], 1, 2)), what
    lab = np.asarray(labels_out)
    assert np.all(lab[c:] == -1) and np.all((lab[:c] >= 0) & (lab[:c] < K)), (what, lab)
    assert np.array_equal(np.bincount(lab[:c], minlength=MIX_MAX)[:MIX_MAX], rec["count"]), (what, rec["count"])
    free = close_calls(f64)
    differ = lab[:c] != f64.labels
    assert not np.any(differ & ~free), (what, "labels", np.flatnonzero(differ & ~free))
    assert np.all(np.abs(rec["count"].astype(int) - f64.count.astype(int)) <= int(free.sum())), (what, rec["count"], f64.count)
    return worst
