"""Shared cases of the belief-query tests (tests/test_beliefquery.py on the CPU, tests/test_gpu_beliefquery.py on the device):
closed forms, the queries a belief is evaluated at, the pairs an mmd is taken of, and the criteria.

The criteria (the definitions are DESIGN.md 3 / incrementalinference.jl_amd/beliefquery.py):

  density    |dev - ref| <= 1e-12 ref + 1e-300 against density_numpy (exact sums).  Derived, not measured: each term carries at
             most a few ulp (exp_nonpos is held to 1.5 ulp by tests/test_nbp_math.py; the error of the argument contributes at
             most (2/e) eps of the largest possible term); a serial sum of c <= 512 non-negative terms adds at most
             c 2^-53 ~ 6e-14 relative.  It is the bound tests/test_gpu_ppe.py uses for the same sum.  (A query far from every
             point has no term near 1 to be relative to: there the three roundings of an exponent a <= 700 -- (q - x) r against
             (q - x) / h, the square, the sum -- move its term by <= 700 * 3 * 2^-53 ~ 2.3e-13 relative, still inside.)  1e-300: a term below
             exp(-700) enters the device's sum as ~1e-304 where the exact value underflows towards 0.
  mmd        |dev - ref| <= 1e-12 absolute against mmd_numpy (exact sums).  Derived: each normalised sum is a mean of terms in
             [0, 1]; a lane's serial sum of at most 512 such terms, divided by its count, errs by at most 512 2^-53 ~ 5.7e-14;
             block_sum and exp add a few 1e-16; the three sums enter with weights 1, 1 and 2: at most 2.4e-13.
"""
import math

import numpy as np

import ppe_cases as pc
from parity_utils import abi, iif

bq = iif.beliefquery
MANIFOLDS = pc.MANIFOLDS
DENS_RTOL, DENS_ATOL = 1e-12, 1e-300
MMD_ATOL = 1e-12
TILE = 256  # NBP_QUERY_TILE of csrc/nbp_query.h: the queries of one belief that one workgroup takes


def gauss_pdf(x, h):
    """the pdf of a zero-mean Gaussian with standard deviations h (one per coordinate) at x"""
    x, h = np.atleast_1d(np.asarray(x, dtype=float)), np.atleast_1d(np.asarray(h, dtype=float))
    return math.exp(-0.5 * math.fsum(((x / h) ** 2).tolist())) / math.prod((math.sqrt(2 * math.pi) * h).tolist())


def mmd_two_points(d, sigma):
    """two one-point beliefs at distance d"""
    return 2 - 2 * math.exp(-sigma * d * d)


def make_queries(manifold, X, bw, nq, rng):
    """nq queries (tangent coordinates) for the belief X, bw, cycling through: the belief's own points, points 1-3 h away,
    points 40 h away (every term underflows) and, on circular coordinates, +-pi"""
    D = abi.MANIFOLD_DIM[manifold]
    Q = np.zeros((nq, D))
    for i in range(nq):
        x = X[rng.integers(len(X))]
        kind = i % 4
        if kind == 0:
            Q[i] = x
        elif kind == 1:
            Q[i] = x + rng.uniform(1, 3, D) * bw * rng.choice([-1.0, 1.0], D)
        elif kind == 2:
            Q[i] = x + 40.0 * bw
        else:
            Q[i] = x + rng.normal(0, 1, D) * bw
            for d in pc.circular_coords(manifold):
                Q[i, d] = (np.pi, -np.pi)[(i // 4) % 2]
    return Q


def check_density(manifold, X, bw, Q, dev, what=""):
    ref = bq.density_numpy(manifold, X, bw, Q)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    if len(ref):
        err = np.abs(dev - ref)
        rel = np.max(err / np.maximum(ref, 1e-280))
        print(f"{what} q={len(ref)}: density in [{ref.min():.3e}, {ref.max():.3e}], max |dev - ref| / ref = {rel:.3e}, "
              f"max |dev - ref| where ref < 1e-280 = {np.max(np.where(ref < 1e-280, err, 0.0)):.3e}")
        assert np.all(err <= DENS_RTOL * ref + DENS_ATOL), (what, dev, ref)
    return ref


def check_mmd(manifold, A, B, sigma, dev, what=""):
    ref = bq.mmd_numpy(manifold, A, B, sigma)
    print(f"{what} sigma={sigma}: mmd dev {dev:.17g} ref {ref:.17g} |diff| {abs(dev - ref):.3e}")
    assert abs(dev - ref) <= MMD_ATOL, (what, dev, ref)
    return ref


def chain6(seed, N=100):
    """x0 .. x5 on the line: a prior on x0 and five odometry steps of 1"""
    fg = iif.initfg(iif.SolverParams(N=N))
    for i in range(6):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
    iif.addFactor(fg, ["x0"], iif.Prior(iif.Normal(0.0, 0.1)))
    for i in range(5):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.Normal(1.0, 0.1)))
    return fg
