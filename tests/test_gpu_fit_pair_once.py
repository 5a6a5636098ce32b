"""-m gpu: one-row fit workgroups visit every pair of points in full chunks of 64 once in their single-precision evaluations
(csrc/nbp_lcv_pairs.h, neg_loo_ll_f32).  The fitted bandwidths must be the oracle's all-double search's and the same launch's
under NBP_FIT_F64=1, bit for bit, at the smallest sizes that take each path of the schedule:

    2, 63    no full chunk                     128   even W: the shared half block
    64       diagonal block only               136   W = 2 plus a partial chunk
    65       one-point partial chunk           200   the workload: W = 3 plus 8
    96, 97   re-deal limit of the partial wave 256   W = 4, no partial chunk
                                               300   must still take the five-wave path

N is the number of points of the beliefs; the slot holds max(N, 8), the smallest a context takes.  The one-row geometry is forced through the context's launch-size threshold (NBP_LCV_P1_MIN=0)."""
import os

import numpy as np
import pytest

from parity_utils import abi, iif

pytestmark = pytest.mark.gpu

SIZES = [2, 63, 64, 65, 96, 97, 128, 136, 200, 256, 300]
MANIFOLDS = [abi.EUCLID1, abi.EUCLID2, abi.CIRCULAR, abi.SE2]


def cloud(rng, manifold, n, kind):
    D = abi.MANIFOLD_DIM[manifold]
    eucl = manifold not in (abi.CIRCULAR, abi.SE2)
    if kind == "gauss":
        c = rng.normal(size=(n, D)) * rng.uniform(0.05, 3.0)
    elif kind == "modes":  # two separated modes: single precision decides every comparison it is asked
        c = rng.normal(size=(n, D)) * 0.05 + np.where(np.arange(n) % 2, 1.3, -1.3)[:, None]
    elif kind == "duplicates":
        c = np.repeat(rng.normal(size=((n + 3) // 4, D)), 4, axis=0)[:n]
    elif kind == "isolated":  # one point far from all others: its sum underflows at small bandwidths (NaN -> double precision)
        c = rng.normal(size=(n, D)) * 0.02
        c[n // 2] += 3.0
    elif kind == "heavy":
        c = rng.standard_cauchy(size=(n, D)) * (1.0 if eucl else 0.2)
    else:  # "offset": 1e6 from the origin (the positions; an angle has no offset)
        c = rng.normal(size=(n, D)) * 0.3
        c[:, : (D if eucl else 2 if manifold == abi.SE2 else 0)] += 1e6
    if manifold == abi.SE2:
        th = c[:, 2]
        return np.stack([c[:, 0], c[:, 1], np.cos(th), np.sin(th), -np.sin(th), np.cos(th)], axis=1)
    if manifold == abi.CIRCULAR:
        return (c + np.pi) % (2 * np.pi) - np.pi
    return c


def write(be, s, manifold, b, N):
    if len(b) == N:
        be.slot_write(s, manifold, b)
    else:  # a belief that holds fewer points than its slot
        be.belief_write(s, manifold, b, np.ones(abi.MANIFOLD_DIM[manifold]))


def device_fit(N, manifold, beliefs, f64):
    N = max(N, 8)  # the slot's capacity
    keys = ("NBP_FIT_F64", "NBP_NO_SPECULATIVE_FITS", "NBP_LCV_P1_MIN")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(NBP_FIT_F64="1" if f64 else "0", NBP_NO_SPECULATIVE_FITS="1", NBP_LCV_P1_MIN="0")
    try:
        be = iif.HipBackend(N, len(beliefs), 0)
        try:
            for s, b in enumerate(beliefs):
                write(be, s, manifold, b, N)
            be.diag(reset=True)
            be.run_bandwidth(list(range(len(beliefs))), [manifold] * len(beliefs))
            return np.array([be.slot_read(s, manifold)[1] for s in range(len(beliefs))]), be.diag()
        finally:
            be.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def oracle_fit(oracle_backend, N, manifold, beliefs):
    N = max(N, 8)
    ob = oracle_backend(N, len(beliefs))
    try:
        for s, b in enumerate(beliefs):
            ob.belief_write(s, manifold, b, np.ones(abi.MANIFOLD_DIM[manifold]))
        ob.run_bandwidth(list(range(len(beliefs))), [manifold] * len(beliefs))
        return np.array([ob.belief_read(s, manifold)[1] for s in range(len(beliefs))])
    finally:
        ob.close()


@pytest.mark.parametrize("manifold", MANIFOLDS)
@pytest.mark.parametrize("N", SIZES)
def test_pair_once_fits_select_the_all_double_bandwidths(oracle_backend, manifold, N):
    rng = np.random.default_rng(7000 + 10 * N + manifold)
    gauss = [cloud(rng, manifold, N, "gauss") for _ in range(3)]
    others = [cloud(rng, manifold, N, k) for k in ("modes", "duplicates", "isolated", "heavy", "offset")]
    if N > 2:  # fewer points than the slot: idle lanes in the last wave, and (N >= 128) a wave without a point
        others += [cloud(rng, manifold, n, "gauss") for n in sorted({N - 1, max(2, N - 70)})]
    for beliefs, is_gauss in ((gauss, True), (others, False)):
        want = oracle_fit(oracle_backend, N, manifold, beliefs)
        f64, d64 = device_fit(N, manifold, beliefs, True)
        f32, d32 = device_fit(N, manifold, beliefs, False)
        print(f"N={N} manifold={manifold} gauss={is_gauss}: evals f64-only {d64['lcv_evals']}, bracketed {d32['lcv_evals']} + {d32['lcv_evals_f32']} single")
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        assert np.array_equal(f32, want), (f32, want)
        assert np.array_equal(f32, f64), (f32, f64)
        assert d64["lcv_evals_f32"] == 0
        if is_gauss:
            assert d32["lcv_evals_f32"] > 0  # no silent fall-back to the all-double search
