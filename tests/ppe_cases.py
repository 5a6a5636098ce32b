"""Shared cases of the point-estimate tests (tests/test_ppe.py on the CPU, tests/test_gpu_ppe.py on the device): the clouds,
and the criteria an estimate is held to.

The criteria (the definition is DESIGN.md 3 / incrementalinference.jl_amd/ppe.py):

  mean       Euclid(1-3) and Circular: the bits of the CPU checker's device-order mean (orc_mean_geodesic_device_order) of the
             coordinates read back from the slot -- the same device function in the same workgroup shape the stage-wise
             parity suite holds to the checker bit for bit.  SE(2): within 1e-13 per coordinate (the heading passes through
             the rotation-matrix host form on its way in and out: an ulp of input).
  max        max_index in [0, c); max = point max_index of the belief as read back (SE(2): x, y bitwise, theta within 1e-15);
             under the float64 densities of the numpy restatement p[max_index] >= (1 - 1e-12) max(p).
             1e-12: the device's exp carries <= ~3e-15 relative error on the terms that matter (exp_nonpos, nbp_device.h), a
             sum of <= 512 positive terms adds <= 512 * 2^-53 ~ 6e-14; 1e-12 is an order of magnitude above the two together.
  beyond D   output entries D .. 2 are zero.
"""
import ctypes as C

import numpy as np

from parity_utils import abi, iif

ppe = iif.ppe
MANIFOLDS = (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3, abi.CIRCULAR, abi.SE2)
CLOUDS = ("gaussian", "two_cluster", "around_circle", "across_pi", "identical")
MAX_RTOL = 1e-12


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def circular_coords(manifold):
    return [d for d in range(abi.MANIFOLD_DIM[manifold]) if (manifold == abi.CIRCULAR and d == 0) or (manifold == abi.SE2 and d == 2)]


def cloud(kind, manifold, n, rng):
    """tangent coordinates (n x D) of one cloud; circular coordinates already wrapped to [-pi, pi)"""
    D = abi.MANIFOLD_DIM[manifold]
    if kind == "gaussian":
        X = rng.normal(0.3, 0.5, (n, D))
    elif kind == "two_cluster":  # 70 / 30, the clusters 10 sigma apart in every coordinate
        heavy = rng.uniform(size=n) < 0.7
        if n >= 2:
            heavy[0], heavy[1] = True, False
        X = np.where(heavy[:, None], -1.0, 1.0) + rng.normal(0, 0.2, (n, D))
    elif kind == "around_circle":  # uniform over the circle: the lift path of the circular mean
        X = rng.uniform(-np.pi, np.pi, (n, D))
    elif kind == "across_pi":  # one cluster that straddles +-pi
        X = rng.normal(np.pi, 0.3, (n, D))
    elif kind == "identical":
        X = np.tile(rng.normal(0.2, 0.5, (1, D)), (n, 1))
    else:
        raise KeyError(kind)
    if kind in ("around_circle", "across_pi"):
        X = wrap(X)  # every coordinate: Euclidean ones are then "written already wrapped" too
    for d in circular_coords(manifold):
        X[:, d] = wrap(X[:, d])
    return np.ascontiguousarray(X)


def to_points(manifold, X):
    """tangent coordinates -> host points (SE(2): x, y, R column-major)"""
    if manifold == abi.SE2:
        c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
        return np.stack([X[:, 0], X[:, 1], c, s, -s, c], axis=1)
    return np.ascontiguousarray(X)


def hand_bandwidth(manifold):
    return np.array([0.3, 0.4, 0.2])[:abi.MANIFOLD_DIM[manifold]]


def oracle_mean(manifold, X):
    """the CPU checker's device-order mean, coordinate by coordinate"""
    from oracle import oracle_backend as ob
    L = ob.lib()
    dp = C.POINTER(C.c_double)
    out = []
    for d in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, d])
        out.append(L.orc_mean_geodesic_device_order(x.ctypes.data_as(dp), len(x), int(d in circular_coords(manifold))))
    return np.array(out)


def check_mean(manifold, X, mean, what=""):
    D = abi.MANIFOLD_DIM[manifold]
    want = oracle_mean(manifold, X)
    print(f"{what} mean: got {mean[:D]}, checker {want}, max |diff| {np.abs(mean[:D] - want).max():.3e}")
    if manifold == abi.SE2:
        d = mean[:D] - want
        d[2] = wrap(d[2])
        assert np.abs(d).max() <= 1e-13, (what, mean, want)
    else:
        assert np.array_equal(mean[:D], want), (what, mean, want, mean[:D] - want)
    assert np.all(mean[D:] == 0), (what, mean)


def check_max(manifold, X, bw, mx, idx, what="", want_index=None):
    """the three criteria of `max`; want_index: the index itself must match (clouds whose runner-up is far below)"""
    D, c = abi.MANIFOLD_DIM[manifold], X.shape[0]
    assert 0 <= idx < c, (what, idx, c)
    if manifold == abi.SE2:
        assert np.array_equal(mx[:2], X[idx, :2]) and abs(wrap(mx[2] - X[idx, 2])) <= 1e-15, (what, mx, X[idx])
    else:
        assert np.array_equal(mx[:D], X[idx]), (what, mx, X[idx])
    assert np.all(mx[D:] == 0), (what, mx)
    p = ppe.kde_density(manifold, X, bw)
    print(f"{what} max: index {idx} (numpy argmax {int(np.argmax(p))}), p[index] / max(p) - 1 = {p[idx] / p.max() - 1:.3e}")
    assert p[idx] >= (1 - MAX_RTOL) * p.max(), (what, idx, int(np.argmax(p)), p[idx], p.max())
    if want_index is not None:
        assert idx == want_index, (what, idx, want_index)


def runner_up_gap(p):
    """relative distance of the second greatest density below the greatest"""
    s = np.sort(p)
    return (s[-1] - s[-2]) / s[-1]
