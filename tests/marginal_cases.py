"""Shared cases of the marginal-density tests (tests/test_marginal.py on the CPU, tests/test_gpu_marginal.py on the device): the
coordinate subsets, the grid sizes, the extents and the criteria.

The criteria (the definitions are DESIGN.md 3 / incrementalinference.jl_amd/marginal.py):

  grid       |dev - ref| <= DENS_RTOL ref + floor against marginal_grid_numpy (exact sums of the separable products), DENS_RTOL =
             1e-12 of tests/query_cases.py: the same sum of the same terms as the density there, a product of two exponentials
             (a few ulp) in place of one.  floor = c 2e-304 / norm: a term below exp(-700) enters the device's sum as ~1e-304 (the
             clamp of exp_nonpos, at most one clamped factor times a factor <= 1 per particle) where numpy's underflows towards 0.
             Explicit extents stay within +-40 h of the cloud so that this floor is the only absolute allowance.
  full set   K = all coordinates of a 1-D or 2-D manifold: density_numpy at the grid points within DENS_RTOL, DENS_ATOL (the
             separable and the summed-exponent forms differ by a few ulp per term).
  mass       sum * step0 * step1 in [1 - 2e-4, 1 + 1e-9] at margin = 4 and a step <= 0.7 h: the tails cut off at 4 h hold at most
             2 Q(4) = 6.3e-5 per Euclidean axis; a trapezoid sum of a Gaussian mixture at that step errs by far less.
"""
import itertools

import numpy as np

import ppe_cases as pc
import query_cases as qc
from parity_utils import abi, coords, iif

mg = iif.marginal
DENS_RTOL, DENS_ATOL = qc.DENS_RTOL, qc.DENS_ATOL
SIZES_1D = [(1,), (17,), (257,)]
SIZES_2D = [(1, 1), (1, 17), (16, 16), (17, 33), (64, 64)]
MASS_LO, MASS_HI = 1 - 2e-4, 1 + 1e-9
KINDS = ("gaussian", "across_pi", "around_circle", "identical")


def subsets(manifold):
    """every 1-element subset and every ordered pair of the manifold's coordinates (0-based)"""
    D = abi.MANIFOLD_DIM[manifold]
    return [(d,) for d in range(D)] + list(itertools.permutations(range(D), 2))


def explicit_extent(manifold, X, bw, dims, n, rng):
    """(lo, step) per axis, flat: a Euclidean axis from up to 3 h below the cloud to up to 3 h above it; a circular axis a full
    turn from a random start (the grid crosses +-pi)"""
    ext = []
    for a, d in enumerate(dims):
        if d in pc.circular_coords(manifold):
            ext += [-np.pi + rng.uniform(0, 1), 2 * np.pi / n[a]]
        else:
            lo, hi = X[:, d].min() - rng.uniform(1, 3) * bw[d], X[:, d].max() + rng.uniform(1, 3) * bw[d]
            ext += [lo, (hi - lo) / max(n[a] - 1, 1)]
    return ext


def floor(c, bw, dims):
    return c * 2e-304 / (c * np.prod([np.sqrt(2 * np.pi) * bw[d] for d in dims]))


def check_grid(manifold, X, bw, dims, n, ext, dev, what=""):
    """dev against marginal_grid_numpy on the explicit extent `ext` (flat lo, step per axis)"""
    ref, _ = mg.marginal_grid_numpy(manifold, X, bw, dims, n, ext[0::2], ext[1::2])
    assert dev.shape == ref.shape == tuple(n), (what, dev.shape, ref.shape)
    err = np.abs(dev - ref)
    fl = floor(len(X), bw, dims)
    print(f"{what} dims={dims} n={n}: ref in [{ref.min():.3e}, {ref.max():.3e}], max |dev - ref| / max(ref, 1e-280) = "
          f"{np.max(err / np.maximum(ref, 1e-280)):.3e}, floor {fl:.3e}")
    assert np.all(err <= DENS_RTOL * ref + fl), (what, dims, n, np.max(err), dev, ref)
    return ref


def load(be, items, seed, first_slot=0):
    """items = [(manifold, cloud kind, count)] -> slot first_slot + i holds belief i, its bandwidth fitted on the device where the
    belief holds more than two points that are not all identical; returns (slots, manifolds, [(X, bw)]) as read back"""
    rng = np.random.default_rng(seed)
    slots, mans = list(range(first_slot, first_slot + len(items))), [m for m, _, _ in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, pc.cloud(kind, m, c, rng)), pc.hand_bandwidth(m), None) for m, kind, c in items])
    fit = [i for i, (m, kind, c) in enumerate(items) if kind != "identical" and c > 2]
    if fit:
        be.run_bandwidth([slots[i] for i in fit], [mans[i] for i in fit])
    back = be.beliefs_read(slots, mans)
    for (pts, bw, _), (m, kind, c) in zip(back, items):
        assert len(pts) == c
    return slots, mans, [(coords(m, pts), bw) for (pts, bw, _), m in zip(back, mans)]


def grid_points(manifold, axes, dims):
    """the grid's own points as queries (q x D; coordinates outside dims zero), row-major with the first axis slowest"""
    D = abi.MANIFOLD_DIM[manifold]
    mesh = np.meshgrid(*axes, indexing="ij")
    Q = np.zeros((mesh[0].size, D))
    for a, d in enumerate(dims):
        Q[:, d] = mesh[a].reshape(-1)
    return Q
