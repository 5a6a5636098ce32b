"""Shared cases of the belief-statistics tests (tests/test_beliefstats.py on the CPU, tests/test_gpu_beliefstats.py on the device):
the clouds (those of ppe_cases), the pairs, and the criteria a result is held to.

The criteria (derived, not measured; the definition is DESIGN.md 3 / incrementalinference.jl_amd/beliefstats.py):

  mean        `mean_out.tobytes()` equals run_ppe's mean of the same slots: one device function in one workgroup shape.
  covariance  against meancov_numpy(X, mean = the device's mean) on the coordinates read back from the slot; with
              A = sum_i |delta_id delta_ie| / (c - 1) and B = sum_i (|delta_id| + |delta_ie|) / (c - 1):
                Euclid(1-3), circle:  |dev - ref| <= 1e-13 A + 1e-300.  The device forms delta by the subtraction (and the wrap)
                  numpy forms it by, rounds each product once as numpy does, adds c of them (wave butterfly + wave partials: at
                  most c roundings of 2^-53 relative to the sum of magnitudes) and divides once; numpy's sum is exact and its
                  division rounds once.  c + 4 roundings of 2^-53 at c <= 512: 5.7e-14.
                SE(2):                |dev - ref| <= 1e-12 A + 4e-15 B.  The heading comes back through cos / sin and atan2: an
                  ulp of theta per point (and of the mean), |theta| <= pi: 4.4e-16 each way, which moves a product by
                  <= 4e-15 (|delta_d| + |delta_e|) between the slot's theta and the theta read back.
              cov[d][e] and cov[e][d] are the same bits; diagonals >= 0; entries beyond D are zero; c < 2: NaN block.
  kld         |dev - ref| <= 1e-12 (1 + |Eaa| + |Eab|) against kld_numpy on the beliefs read back.  exp_nonpos carries ~3e-15
              relative error, a sum of <= 512 positive terms 512 * 2^-53 ~ 6e-14, nbpm_log one ulp, the exponent e_j a few ulps of
              itself (it enters M, and M enters l, at full size: hence the bound relative to the terms); 1e-12 is an order of
              magnitude above these together.
  wrap        a CONDITION of the comparison, not a measurement: no |x - mean| (beliefs; the device's mean) and no |a_i - y_j|
              (pairs; a against a and a against b) on a circular coordinate lies within 1e-9 of pi.  Inside that margin the
              wrap's branch could differ between the device and numpy.  Each test asserts it before comparing;
              tests/test_beliefstats.py asserts on the CPU, with meancov_numpy's own mean, that the seeds used meet it (1e-9 is a
              million times the agreement of the two means).
"""
import numpy as np

import ppe_cases as pc
from parity_utils import abi, coords, iif

bs = iif.beliefstats
MANIFOLDS = pc.MANIFOLDS
WRAP_MARGIN = 1e-9
KLD_RTOL = 1e-12
FULL_COUNTS = (64, 65, 200, 257, 512)      # test_meancov_every_manifold_and_cloud_at_full_count: seed 100 + N
BELOW_COUNTS = (1, 2, 63, 150)             # test_meancov_counts_below_the_context_size: N = 200, seed 7
BELOW_CLOUDS = ("gaussian", "across_pi", "around_circle", "identical")
KLD_SIZES = (64, 65, 200, 512)             # test_kld_every_manifold: seed 300 + N


def full_items(N):
    return [(m, kind, N) for m in MANIFOLDS for kind in pc.CLOUDS]


def below_items():
    return [(m, kind, c) for m in MANIFOLDS for c in BELOW_COUNTS for kind in BELOW_CLOUDS]


def batch_items(n, N, seed):
    rng = np.random.default_rng(seed)
    return [(MANIFOLDS[rng.integers(5)], pc.CLOUDS[rng.integers(5)], int(rng.choice([N, N, N, 150, 63, 2, 1]))) for _ in range(n)]


def clouds(items, seed):
    """items = [(manifold, cloud kind, count)] -> tangent coordinates, one array per item, drawn in order from one generator"""
    rng = np.random.default_rng(seed)
    return [pc.cloud(kind, m, c, rng) for m, kind, c in items]


def load(be, items, seed, first_slot=0, fit=False):
    """slot first_slot + i holds belief i with the hand bandwidth (fit: nbp_run_bandwidth where the count allows a fit)"""
    Xs = clouds(items, seed)
    slots, mans = list(range(first_slot, first_slot + len(items))), [m for m, _, _ in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), pc.hand_bandwidth(m), None) for m, X in zip(mans, Xs)])
    if fit:
        idx = [i for i, (m, kind, c) in enumerate(items) if kind != "identical" and c > 2]
        if idx:
            be.run_bandwidth([slots[i] for i in idx], [mans[i] for i in idx])
    return slots, mans


# ---- the wrap condition ----------------------------------------------------------------------------------------------------
def belief_wrap_margin(manifold, X, mean):
    """the least distance of |x - mean| from pi over the circular coordinates (inf when there is none)"""
    out = np.inf
    for d in pc.circular_coords(manifold):
        out = min(out, float(np.abs(np.abs(X[:, d] - mean[d]) - np.pi).min()))
    return out


def pair_wrap_margin(manifold, A, B):
    """the least distance of |a_i - y_j| from pi over the circular coordinates, y running over a's and b's points"""
    out = np.inf
    for d in pc.circular_coords(manifold):
        for Y in (A, B):
            out = min(out, float(np.abs(np.abs(A[:, d, None] - Y[None, :, d]) - np.pi).min()))
    return out


# ---- covariance ------------------------------------------------------------------------------------------------------------
def check_cov(manifold, pts, mean, cov, what=""):
    """the criteria of a covariance: `pts` the belief as read back (host form), `mean` / `cov` the device's rows (3, 3 x 3)"""
    D, X = abi.MANIFOLD_DIM[manifold], coords(manifold, np.asarray(pts))
    c = X.shape[0]
    assert np.all(cov[D:, :] == 0) and np.all(cov[:, D:] == 0) and np.all(mean[D:] == 0), (what, mean, cov)
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes(), (what, cov)
    if c < 2:
        assert np.isnan(cov[:D, :D]).all(), (what, cov)
        return
    margin = belief_wrap_margin(manifold, X, mean)
    assert margin > WRAP_MARGIN, (what, "wrap condition", margin)
    _, ref = bs.meancov_numpy(manifold, pts, mean=mean[:D])
    delta = X - mean[None, :D]
    for d in pc.circular_coords(manifold):
        delta[:, d] = iif.beliefquery._wrap(delta[:, d])  # (the identity on [-pi, pi), as in meancov_numpy: a tiny delta stays)
    ad = np.abs(delta)
    worst = 0.0
    for d in range(D):
        assert cov[d, d] >= 0, (what, cov)
        for e in range(D):
            A = float((ad[:, d] * ad[:, e]).sum()) / (c - 1)
            B = float((ad[:, d] + ad[:, e]).sum()) / (c - 1)
            bound = 1e-12 * A + 4e-15 * B if manifold == abi.SE2 else 1e-13 * A + 1e-300
            err = abs(cov[d, e] - ref[d, e])
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, (what, d, e, cov[d, e], ref[d, e], err, bound)
    print(f"{what} cov diag {np.diag(cov)[:D]}, worst |dev - ref| / bound {worst:.3f}, wrap margin {margin:.2e}")


# ---- kld -------------------------------------------------------------------------------------------------------------------
def kld_pairs(N):
    """[(manifold, (kind_a, count_a, shift_a), (kind_b, count_b, shift_b))] of test_kld_every_manifold in a context of N points:
    shifted Gaussians, two clusters against a Gaussian, and unequal counts (200 / 63 / 1 where the context holds 200)"""
    big = 200 if N >= 200 else N
    out = []
    for m in MANIFOLDS:
        out += [(m, ("gaussian", N, 0.0), ("gaussian", N, 0.7)),
                (m, ("two_cluster", N, 0.0), ("gaussian", N, 0.0)),
                (m, ("gaussian", big, 0.0), ("gaussian", 63, 0.4)),
                (m, ("gaussian", 1, 0.0), ("gaussian", big, 0.0)),
                (m, ("gaussian", big, 0.0), ("gaussian", 1, 0.0))]
    return out


def mixed_pairs(n, N, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = MANIFOLDS[rng.integers(5)]
        ca, cb = (int(rng.choice([N, N, 150, 63, 2, 1])) for _ in range(2))
        out.append((m, (("gaussian", "two_cluster")[rng.integers(2)], ca, 0.0), ("gaussian", cb, float(rng.choice([0.0, 0.5, 1.5])))))
    return out


def pair_clouds(pairs, seed):
    """-> [(A, B)] tangent coordinates, b shifted by its shift in every coordinate (circular ones wrapped back)"""
    rng = np.random.default_rng(seed)
    out = []
    for m, (ka, ca, sa), (kb, cb, sb) in pairs:
        A, B = pc.cloud(ka, m, ca, rng) + sa, pc.cloud(kb, m, cb, rng) + sb
        for d in pc.circular_coords(m):
            A[:, d], B[:, d] = pc.wrap(A[:, d]), pc.wrap(B[:, d])
        out.append((np.ascontiguousarray(A), np.ascontiguousarray(B)))
    return out


def load_pairs(be, pairs, seed, first_slot=0, fit=True):
    """pair i: a in slot first_slot + 2 i, b in the next; hand bandwidths where the count is below 3 (or fit=False), otherwise
    nbp_run_bandwidth -> (slots_a, slots_b, manifolds)"""
    cl = pair_clouds(pairs, seed)
    slots, mans, bel, fits = [], [], [], []
    for i, ((m, (_, ca, _), (_, cb, _)), (A, B)) in enumerate(zip(pairs, cl)):
        for k, (X, c) in enumerate(((A, ca), (B, cb))):
            s = first_slot + 2 * i + k
            slots.append(s)
            mans.append(m)
            bel.append((pc.to_points(m, X), pc.hand_bandwidth(m), None))
            if fit and c >= 3:
                fits.append((s, m))
    be.beliefs_write(slots, mans, bel)
    if fits:
        be.run_bandwidth([s for s, _ in fits], [m for _, m in fits])
    return slots[0::2], slots[1::2], mans[0::2]


def check_kld(be, sa, sb, mans, val, terms, what=""):
    """every pair of a run_kld against kld_numpy on the beliefs read back"""
    back_a, back_b = be.beliefs_read(sa, mans), be.beliefs_read(sb, mans)
    worst = 0.0
    for i, m in enumerate(mans):
        A, B = coords(m, back_a[i][0]), coords(m, back_b[i][0])
        margin = pair_wrap_margin(m, A, B)
        assert margin > WRAP_MARGIN, (what, i, "wrap condition", margin)
        eaa, eab = bs.kld_terms_numpy(m, A, back_a[i][1], B, back_b[i][1])
        bound = KLD_RTOL * (1 + abs(eaa) + abs(eab))
        print(f"{what}[{i}] manifold {m} counts {len(A)}/{len(B)}: kld {val[i]:.6g} (numpy {eaa - eab:.6g}), Eaa {terms[i, 0]:.6g}, "
              f"Eab {terms[i, 1]:.6g}, |diff| / bound {abs(val[i] - (eaa - eab)) / bound:.3f}")
        assert np.isfinite(val[i]) and abs(val[i] - (eaa - eab)) <= bound, (what, i, val[i], eaa - eab, bound)
        assert abs(terms[i, 0] - eaa) <= bound and abs(terms[i, 1] - eab) <= bound, (what, i, terms[i], eaa, eab)
        assert (terms[i, 0] - terms[i, 1]).tobytes() == val[i].tobytes(), (what, i)
        worst = max(worst, abs(val[i] - (eaa - eab)) / bound)
    return worst
