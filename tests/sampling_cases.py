"""Known answers for every random draw a proposal makes, written once and run on the oracle (test_sampling_known_answers.py)
and on the HIP library (test_gpu_sampling_known_answers.py).  Nothing here compares one backend with the other: the
expected values come from the definitions alone -- a Philox4x32-10 written out below and held to Random123's published
vectors, mpmath at 50 digits, the distributions' own CDFs / pmfs / moments (scipy.stats).

Sample sizes.  One proposal is one workgroup of N <= 512 particles; a case pools a few hundred to 1600 descriptors with
consecutive 64-bit seeds in ONE run_proposals launch (pooling over seeds is part of the test: overlapping counters between
neighbouring seeds would show up as dependence).

Thresholds.  Every statistical assert is a quantile of the statistic's own null distribution at level ALPHA = 1e-4 / BUDGET:
the whole file may raise a false alarm once in 10^4 runs, split evenly over at most BUDGET asserts (the helpers count
themselves; test_false_alarm_budget holds the count to BUDGET).  No threshold is an observed number.  Each statistic is also
fed a numpy sample of the same size from a slightly wrong law in test_sampling_known_answers.py (sigma off by 1 %, a dropped
Cholesky entry, a pmf entry off by 0.01, a last kernel never picked, entropy 2 % narrow, lag-1 correlation 0.01, a label
leaking into 1 % of the values) and must reject it."""
import numpy as np
from scipy import stats

from parity_utils import abi, coords

# ---- the stream layout under test (DESIGN.md "RNG", seeds.py): counter (n, purpose, k, NBP_TAG), key = the op's seed -----------
NBP_TAG = 0x4E4250
PURP_MEAS, PURP_MIXLBL, PURP_HYPO, PURP_ENTROPY, PURP_KDESEL, PURP_KDENOISE = 1, 2, 3, 4, 5, 6
PURP_ANYN, PURP_OLDSEL, PURP_OLDNOISE = 11, 12, 13
_M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), from the paper"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


# Random123's known-answer vectors (kat_vectors, philox4x32 10 rounds): counter x4, key x2 -> output x4
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((_M32,) * 4, (_M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def uniform_pair(seed, n, purpose, k):
    """the two uniforms of block (n, purpose, k) of the op keyed `seed`: 53 bits of each 64-bit half, centred in its cell"""
    o = philox4x32_10((n, purpose, k, NBP_TAG), (seed & _M32, (seed >> 32) & _M32))
    return (((o[1] << 32 | o[0]) >> 11) + 0.5) / 2.0 ** 53, (((o[3] << 32 | o[2]) >> 11) + 0.5) / 2.0 ** 53


# ---- the false-alarm budget ------------------------------------------------------------------------------------------------------
ALPHA_FILE = 1e-4
BUDGET = 2500
ALPHA = ALPHA_FILE / BUDGET
spent = [0]  # statistical asserts made so far in this process


def _spend():
    """every statistical assert passes through here: the budget holds in any order of the tests, under -k and in every worker
    of a split run (a process can only spend less than the whole file).  Counts of a full run: the CPU leg 924 (399 in the
    oracle's cases, 525 in the power checks), the GPU leg 399 (the cases alone)."""
    spent[0] += 1
    assert spent[0] <= BUDGET, f"{spent[0]} statistical asserts: ALPHA = {ALPHA_FILE} / {BUDGET} no longer covers the file"


collected = None  # a list while a power check wants to see EVERY statistic that rejects, not the first one


def _check(ok, msg):
    if not ok:
        if collected is None:
            raise AssertionError(msg)
        collected.append(msg)


def z_ok(z, what):
    """z ~ N(0, 1) under the null (exactly standardised: known mean and standard error); two-sided quantile"""
    _spend()
    thr = stats.norm.isf(ALPHA / 2)
    _check(abs(z) < thr, f"{what}: z = {z:.2f}, two-sided N(0,1) quantile at {ALPHA:.1e} is {thr:.2f}")


def ks_ok(x, cdf, what):
    """Kolmogorov-Smirnov D_n against the exact CDF; threshold = the quantile of D_n's own distribution (scipy.stats.kstwo)"""
    _spend()
    x = np.sort(np.asarray(x, dtype=float).ravel())
    n = x.size
    F = cdf(x)
    D = max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(n) / n).max())
    thr = stats.kstwo.isf(ALPHA, n)
    _check(D < thr, f"{what}: D_n = {D:.5f} (n = {n}), kstwo quantile at {ALPHA:.1e} is {thr:.5f}")


def chi2_ok(counts, probs, what):
    """Pearson chi-square of counts against exact cell probabilities (a fully specified null: dof = cells - 1).  A cell of
    probability zero must be empty -- exactly, no statistics; cells expecting fewer than 5 are merged into one."""
    counts, probs = np.asarray(counts, dtype=float).ravel(), np.asarray(probs, dtype=float).ravel()
    assert counts[probs == 0].sum() == 0, f"{what}: {int(counts[probs == 0].sum())} draws of a zero-probability cell"
    n = counts.sum()
    c, e = counts[probs > 0], probs[probs > 0] * n
    small = e < 5
    if small.any():
        c, e = np.append(c[~small], c[small].sum()), np.append(e[~small], e[small].sum())
    if c.size < 2:
        return
    _spend()
    x2 = float(((c - e) ** 2 / e).sum())
    thr = stats.chi2.isf(ALPHA, c.size - 1)
    _check(x2 < thr, f"{what}: chi2 = {x2:.1f} (dof {c.size - 1}, n = {int(n)}), quantile at {ALPHA:.1e} is {thr:.1f}")


def table_ok(qa, qb, what, k=8):
    """independence of two samples given as exact quantiles in (0, 1): the k x k table of quantile pairs has probability
    1 / k^2 per cell (both margins are known: fully specified, dof k^2 - 1)"""
    ia, ib = np.minimum((qa * k).astype(int), k - 1), np.minimum((qb * k).astype(int), k - 1)
    chi2_ok(np.bincount(ia * k + ib, minlength=k * k), np.full(k * k, 1.0 / (k * k)), what)


def corr_ok(a, b, what):
    """a, b standardised with their KNOWN means and variances: under independence mean(a b) sqrt(n) has mean 0, variance
    exactly 1, and is normal by the CLT at n >= 10^5"""
    z_ok(float(np.mean(a * b) * np.sqrt(a.size)), what)


def independent_uniforms_ok(qa, qb, what):
    s12 = np.sqrt(12.0)
    corr_ok((qa - 0.5) * s12, (qb - 0.5) * s12, what + ": correlation")
    table_ok(qa, qb, what + ": 8x8 quantile table")


# ---- batteries: one per law, shared by the backend cases and by the power checks -------------------------------------------------
def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def gaussian_ok(x, mu, L, what, circ=()):
    """x (n, D) against N(mu, L L'): means and every covariance entry as z-scores with their exact standard errors
    (Var(mean_i) = S_ii / n; Var of a product of centred normals = S_ii S_jj + S_ij^2, Isserlis), KS and second moments of
    the coordinates whitened by inv(L) against N(0, I), and the 8x8 quantile table of every pair of whitened coordinates.  Circular
    coordinates are unwrapped about the mean: the draws' sigma keeps the mass beyond +-pi from it below 1e-20."""
    mu, L = np.asarray(mu, dtype=float), np.asarray(L, dtype=float)
    n, D = x.shape
    S = L @ L.T
    c = x - mu
    for d in circ:
        c[:, d] = wrap(c[:, d])
    for i in range(D):
        z_ok(float(c[:, i].mean() / np.sqrt(S[i, i] / n)), f"{what}: mean[{i}]")
        for j in range(i + 1):
            z_ok(float((np.mean(c[:, i] * c[:, j]) - S[i, j]) / np.sqrt((S[i, i] * S[j, j] + S[i, j] ** 2) / n)), f"{what}: cov[{i},{j}]")
    w = np.linalg.solve(L, c.T).T
    q = stats.norm.cdf(w)
    for i in range(D):
        ks_ok(w[:, i], stats.norm.cdf, f"{what}: whitened coordinate {i}")
        # E[w_i w_j] = delta_ij with s.e. sqrt(2 / n) on the diagonal, 1 / sqrt(n) off it: sees a 1 % error of ANY entry of L,
        # also one that the covariance entries above, dominated by a larger entry of the same row, do not
        for j in range(i + 1):
            z_ok(float((np.mean(w[:, i] * w[:, j]) - (i == j)) * np.sqrt(n / (2.0 if i == j else 1.0))), f"{what}: whitened moment[{i},{j}]")
        for j in range(i):
            table_ok(q[:, i], q[:, j], f"{what}: whitened coordinates ({j},{i})")


def uniform_ok(x, a, b, what):
    """U(a, b): support, KS, mean (s.e. (b-a)/sqrt(12 n))"""
    assert x.min() >= a and x.max() <= b, what
    ks_ok(x, lambda t: (t - a) / (b - a), what + ": KS")
    z_ok(float((x.mean() - (a + b) / 2) / ((b - a) / np.sqrt(12.0 * x.size))), what + ": mean")


def rayleigh_ok(x, s, what):
    """Rayleigh(s): KS against 1 - exp(-x^2 / 2 s^2); x^2 / 2 s^2 ~ Exp(1): mean 1, s.e. 1 / sqrt(n)"""
    assert x.min() > 0, what
    ks_ok(x, lambda t: -np.expm1(-t * t / (2 * s * s)), what + ": KS")
    z_ok(float((np.mean(x * x) / (2 * s * s) - 1.0) * np.sqrt(x.size)), what + ": second moment")


def unit_entropy_ok(e, what):
    """e (n, D) = (out - old) / (spreadNH * spread) of the null particles: U(-1/2, 1/2) on every coordinate (support to
    1e-12: the spread is recomputed here with another summation order), KS, coordinates pairwise independent"""
    assert np.abs(e).max() <= 0.5 * (1 + 1e-12), f"{what}: |entropy| up to {np.abs(e).max()} of the width"
    for i in range(e.shape[1]):
        ks_ok(e[:, i], lambda t: t + 0.5, f"{what}: coordinate {i}")
        for j in range(i):
            independent_uniforms_ok(e[:, i] + 0.5, e[:, j] + 0.5, f"{what}: coordinates ({j},{i})")


def kernel_pick_ok(idx, cd, what):
    """the picked kernel is uniform over the cd points of the density; both ends must be reachable"""
    cnt = np.bincount(idx, minlength=cd)
    assert cnt.size == cd, f"{what}: kernel index {idx.max()} beyond the density's {cd} points"
    chi2_ok(cnt, np.full(cd, 1.0 / cd), what + ": kernel counts")
    if idx.size >= 40 * cd:  # P(an end never drawn) <= 2 exp(-40): not a statistical statement at this size
        assert cnt[0] > 0 and cnt[-1] > 0, f"{what}: an end of the density is never picked"


# ---- running proposals in bulk ---------------------------------------------------------------------------------------------------
def prior_desc(manifold, seed, comps, *, kind=abi.F_PRIOR, nullhypo=0.0, mhidx_in=-1, mhidx_out=-1, table_slot=None, msg_slot=None):
    """comps: [(weight, mean, lower Cholesky factor (D x D) or sigmas, family)]; the target's current belief is slot 0"""
    d = abi.ProposalDesc()
    d.factor_kind, d.manifold, d.nvars, d.sfidx = kind, manifold, 1, 0
    d.ncomp, d.inflate_cycles, d.skip_bandwidth = len(comps), 3, 1
    d.mhidx_in, d.mhidx_out = mhidx_in, mhidx_out
    d.inflation, d.spread_nh, d.nullhypo = 5.0, 3.0, nullhypo
    for c, (w, mu, L, fam) in enumerate(comps):
        L = np.asarray(L, dtype=float)
        L = np.diag(L) if L.ndim == 1 else L
        d.comp[c][0] = w
        for i, m in enumerate(mu):
            d.comp[c][1 + i] = m
        for i in range(L.shape[0]):
            for j in range(i + 1):
                d.comp[c][4 + 3 * i + j] = L[i, j]
        if fam:
            d.comp[c][12] = fam
    if table_slot is not None:
        d.var_slot[abi.MAXV - 1] = table_slot
    if msg_slot is not None:
        d.var_slot[1] = msg_slot
    d.seed = seed
    return d


def to_points(manifold, c):
    c = np.asarray(c, dtype=float).reshape(len(c), -1)
    if manifold == abi.SE2:
        return np.stack([c[:, 0], c[:, 1], np.cos(c[:, 2]), np.sin(c[:, 2]), -np.sin(c[:, 2]), np.cos(c[:, 2])], axis=1)
    return c


def run_pool(backend, N, descs, *, n_in=1, setup=None, side_ints=0, side_init=None):
    """all descriptors in ONE launch: descriptor i writes slot n_in + i; slot 0 is the target's current belief (zeros unless
    `setup(be)` writes it).  -> ([coords (N, D) per descriptor], side buffer)"""
    be = backend(N, n_in + len(descs), side_ints)
    try:
        be.slot_write(0, abi.EUCLID3, np.zeros((N, 3)), np.ones(3))
        if setup is not None:
            setup(be)
        if side_init is not None:
            be.side_write(0, side_init)
        for i, d in enumerate(descs):
            d.out_slot = n_in + i
        be.run_proposals(descs)
        out = [coords(d.manifold, be.slot_read(d.out_slot, d.manifold)[0]) for d in descs]
        side = be.side_read(0, side_ints) if side_ints else None
    finally:
        be.close()
    return out, side


SEED0 = 0x9E3779B97F4A7C15  # bits set in both words; a pool takes SEED0 + base, + 1, + 2 ...


def pool_seeds(base, n):
    return [(SEED0 + (base << 40) + i) & (2 ** 64 - 1) for i in range(n)]


# ==================================================================================================================================
# 1. the generator itself, bit for bit
# ==================================================================================================================================
def case_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        assert philox4x32_10(ctr, key) == want, (ctr, key)


STREAM_SEEDS = [1, 0x80000000, 0xFFFFFFFF, 0x100000000, 0xDEADBEEF00000001, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF]
STREAM_N = [1, 8, 37, 64, 200, 512, 1024]  # below, at and beyond the ends of libnbp's range [8, 512]; not multiples of the wave (37, 200)
_RAY_SIGMA = 1.7
_G = {  # Gaussian priors of dimension 1, 2, 3: (mean, lower Cholesky factor)
    abi.EUCLID1: ([0.75], [[1.5]]),
    abi.EUCLID2: ([-2.0, 3.0], [[0.5, 0.0], [1.25, 0.75]]),
    abi.EUCLID3: ([1.0, -4.0, 0.5], [[2.0, 0.0, 0.0], [-1.5, 0.25, 0.0], [0.5, -0.75, 1.25]]),
}


_MP = None


def stream_particle_ok(s, n, uni, ray, gauss):
    """particle n of the op keyed s: `uni` from Prior(Uniform(0, 1)), `ray` from Prior(Rayleigh(_RAY_SIGMA)), gauss[g] the
    point drawn by the g-th Gaussian prior of _G -- against the Python stream, the tolerances derived here"""
    global _MP
    if _MP is None:
        import mpmath
        _MP = mpmath.mp.clone()
        _MP.dps = 50
    mp = _MP
    eps = 2.0 ** -52  # one ulp of a double is at most eps times its magnitude
    ua, ub = uniform_pair(s, n, PURP_MEAS, 0)
    uc, ud = uniform_pair(s, n, PURP_MEAS, 1)
    assert uni == ua, (hex(s), n, "uniform", uni, ua)
    # Rayleigh: sigma * sqrt(-2 log ua).  log within 1 ulp (relative eps; the doubling is exact), the square root
    # halves a relative error and rounds once (eps / 2), the product rounds once (eps / 2): 1.5 eps to first order;
    # 2 eps covers the second-order terms.
    want = _RAY_SIGMA * mp.sqrt(-2 * mp.log(mp.mpf(ua)))
    assert abs(mp.mpf(float(ray)) - want) <= 2 * eps * want, (hex(s), n, "rayleigh", ray, float(want))
    # Box-Muller: n = r (cos, sin)(a), r = sqrt(-2 log u1), a = fl(fl(2 pi) u2).
    #   r: relative eps / 2 (the log's ulp through the square root) + eps / 2 (the root's rounding); taken as 1.5 eps.
    #   a: fl(2 pi) is within eps/2 of 2 pi relatively and the product rounds once: |a - 2 pi u2| <= 2 pi eps, and
    #      |d sin|, |d cos| <= 1, so that much ABSOLUTE error in the functions; sincos itself adds 1 ulp (<= eps, the
    #      values are below 1) + |a| 1e-26 <= 7e-26.  Absolute, not relative: next to a zero of the function.
    #   the product r * c rounds once (eps / 2 relative).
    # |d n| <= r (2 pi eps + eps + 7e-26) + |n| (1.5 eps + eps / 2)
    # The affine map z_i = mu_i + sum_j L_ij n_j: the propagated |L_ij| |d n_j|, plus one rounding per operation (a
    # product and a sum per term, fused or not), each at most eps / 2 of a partial sum bounded by |mu_i| + sum |L_ij n_j|.
    nn = []
    for (u1, u2) in ((ua, ub), (uc, ud)):
        r, a = mp.sqrt(-2 * mp.log(mp.mpf(u1))), 2 * mp.pi * mp.mpf(u2)
        for v in (r * mp.cos(a), r * mp.sin(a)):
            nn.append((v, float(r) * (2 * np.pi * eps + eps + 7e-26) + abs(float(v)) * 2 * eps))
    for g, (mu, L) in zip(gauss, _G.values()):
        for i in range(len(mu)):
            want, tol, mag = mp.mpf(mu[i]), 0.0, abs(mu[i])
            for j in range(i + 1):
                want += mp.mpf(L[i][j]) * nn[j][0]
                tol += abs(L[i][j]) * nn[j][1]
                mag += abs(L[i][j] * float(nn[j][0]))
            tol += 2 * (i + 1) * (eps / 2) * mag
            assert abs(mp.mpf(float(g[i])) - want) <= tol, (hex(s), n, "gaussian", len(mu), i, float(g[i]), float(want), tol)


def case_stream_is_philox(backend, N):
    """Prior(Uniform(0, 1)) without bandwidth fit or null hypothesis outputs fma(1, ua, 0) = ua: particle n IS the first
    uniform of block (n, PURP_MEAS, 0) of the op's seed, exactly.  The Rayleigh prior and the Gaussian priors of dimension 1, 2
    and 3 (both uniforms of block k = 0 and, for D = 3, block k = 1) are predicted from the same Python stream with mpmath at
    50 digits, to the error bounds include/nbp_math.h states for its own functions.

    -> "ran", or "refused" where the backend refuses N with libnbp's documented range error (NBP_MAXN, "N must be in
    [8, 512]", include/nbp.h).  The callers assert which: the oracle runs every N, the library refuses exactly those outside
    its range -- N = 1 and N = 1024 run on the oracle only."""
    descs = []
    for s in STREAM_SEEDS:
        descs.append(prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [1.0], abi.DIST_UNIFORM)]))
        descs.append(prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [_RAY_SIGMA], abi.DIST_RAYLEIGH)]))
        for m, (mu, L) in _G.items():
            descs.append(prior_desc(m, s, [(1.0, mu, L, 0)]))
    try:
        out, _ = run_pool(backend, N, descs)
    except RuntimeError as e:
        assert not 8 <= N <= abi.MAXN and "N must be in [8, 512]" in str(e), (N, str(e))
        return "refused"
    for si, s in enumerate(STREAM_SEEDS):
        o = out[5 * si:5 * si + 5]
        for n in range(N):
            stream_particle_ok(s, n, o[0][n, 0], o[1][n, 0], [o[2 + gi][n] for gi in range(3)])
    return "ran"


# ==================================================================================================================================
# 2. every draw against its distribution
# ==================================================================================================================================
NP = 512     # particles per proposal in the pooled cases
OPS = 1600   # proposals per pool: 819 200 draws -- what the 1 % perturbations need (see the power checks)

GAUSS = {  # manifold -> (mean, lower Cholesky factor, circular coordinates); strong correlation where there is more than one
    abi.EUCLID1: ([2.5], [[0.8]], ()),
    abi.EUCLID2: ([1.0, -2.0], [[1.5, 0.0], [-1.8, 0.4]], ()),
    abi.EUCLID3: ([0.5, 1.5, -1.0], [[1.2, 0.0, 0.0], [1.0, 0.3, 0.0], [-0.9, 0.8, 0.25]], ()),
    abi.CIRCULAR: ([3.0], [[0.3]], (0,)),  # the mass straddles the seam at pi
    abi.SE2: ([4.0, -1.0, -3.05], [[1.0, 0.0, 0.0], [0.9, 0.2, 0.0], [0.2, -0.1, 0.05]], (2,)),
}


def case_gaussian_measurement(backend, manifold):
    mu, L, circ = GAUSS[manifold]
    out, _ = run_pool(backend, NP, [prior_desc(manifold, s, [(1.0, mu, L, 0)]) for s in pool_seeds(manifold, OPS)])
    gaussian_ok(np.concatenate(out), mu, L, f"Gaussian prior on manifold {manifold}", circ)


def case_uniform_and_rayleigh(backend):
    seeds = pool_seeds(11, OPS)
    descs = [prior_desc(abi.EUCLID1, s, [(1.0, [2.0], [3.0], abi.DIST_UNIFORM)]) for s in seeds]
    descs += [prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [_RAY_SIGMA], abi.DIST_RAYLEIGH)]) for s in seeds]
    out, _ = run_pool(backend, NP, descs)
    uniform_ok(np.concatenate(out[:OPS]).ravel(), 2.0, 5.0, "Uniform(2, 5) prior")
    rayleigh_ok(np.concatenate(out[OPS:]).ravel(), _RAY_SIGMA, "Rayleigh(1.7) prior")


def table_pmfs(N):
    """tabulated samplers of K = 2, 30 and N entries, zero weights at the first position, the last and in the middle"""
    rng = np.random.default_rng(21)
    out = {2: np.array([0.3, 0.7])}
    for K in (30, N):
        w = rng.uniform(0.2, 1.0, K)
        w[[0, K // 2, K // 2 + 1, K - 1]] = 0.0
        out[K] = w / w.sum()
    w = rng.uniform(0.2, 1.0, 30)  # and one whose LAST entry is positive and small: it must be drawn
    w[29] = 0.05
    out["30, last positive"] = w / w.sum()
    return out


def case_tabulated(backend):
    pm = table_pmfs(NP)
    ops = 400  # 204 800 draws per table: a pmf entry off by 0.01 moves chi2 by >= n 1e-4 / p ~ 20 / p (power check)
    descs = []

    def setup(be):
        for t, w in enumerate(pm.values()):
            cum = np.cumsum(w)
            cum[-1] = 1.0
            be.belief_write(1 + t, abi.EUCLID2, np.stack([np.arange(1.0, w.size + 1), cum], axis=1), np.ones(2))
    for t in range(len(pm)):
        descs += [prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [1.0], abi.DIST_TABLE)], table_slot=1 + t) for s in pool_seeds(30 + t, ops)]
    out, _ = run_pool(backend, NP, descs, n_in=1 + len(pm), setup=setup)
    for t, (name, w) in enumerate(pm.items()):
        x = np.concatenate(out[t * ops:(t + 1) * ops]).ravel()
        assert np.isin(x, np.arange(1.0, w.size + 1)).all(), name
        cnt = np.bincount(x.astype(int) - 1, minlength=w.size)
        chi2_ok(cnt, w, f"table of {name} entries")
        assert cnt[np.flatnonzero(w)[-1]] > 0, f"table of {name} entries: the last positive entry is never drawn"


MIXTURES = {  # weights; component c is N(100 c, 1): the value names its label
    "2": [0.35, 0.65],
    "3, a zero weight": [0.5, 0.0, 0.5],
    "4 (NBP_MAXC)": [0.1, 0.2, 0.3, 0.4],
    "4, a zero weight last": [0.25, 0.5, 0.25, 0.0],
    # the running double sum of these is 1 - 2^-53 < 1 (asserted in the case): a uniform at or above it, probability 2^-53 per
    # draw, takes the `c = last` fallback.  No pool can make that branch run; what the pool shows is that a short sum does not
    # bias the counts (nor send anything to a component beyond the last)
    "4, sum one ulp short of 1": [0.25, 0.25, 0.25, 0.25 - 2.0 ** -53],
}


def mixture_pmf(w):
    """the law of the label: the weights, what their sum leaves short of 1 falling to the last positive one"""
    w = np.array(w, dtype=float)
    w[np.flatnonzero(w)[-1]] += 1.0 - w.sum()
    return w


def labels_ok(x, w, what):
    """x: draws of the mixture sum_c w_c N(100 c, 1).  Component counts against w (zero weights never), and the label against
    the within-component quantile of the value (drawn under PURP_MIXLBL and PURP_MEAS from one seed) on a (components x 8)
    table with cell probability w_c / 8"""
    lab = np.rint(x / 100.0).astype(int)
    assert lab.min() >= 0 and lab.max() < len(w), what
    q = stats.norm.cdf(x - 100.0 * lab)
    chi2_ok(np.bincount(lab, minlength=len(w)), w, what + ": component counts")
    b = np.minimum((q * 8).astype(int), 7)
    chi2_ok(np.bincount(lab * 8 + b, minlength=8 * len(w)), np.repeat(np.asarray(w) / 8.0, 8), what + ": label x quantile")
    ks_ok(q, lambda t: t, what + ": within-component quantile")


def case_mixture_labels(backend):
    descs = []
    for t, w in enumerate(MIXTURES.values()):
        comps = [(wc, [100.0 * c], [1.0], 0) for c, wc in enumerate(w)]
        descs += [prior_desc(abi.EUCLID1, s, comps) for s in pool_seeds(40 + t, OPS)]
    out, _ = run_pool(backend, NP, descs)
    run = 0.0
    for wc in MIXTURES["4, sum one ulp short of 1"]:
        run += wc  # the order the kernel and the oracle add them in
    assert run == 1.0 - 2.0 ** -53 < 1.0
    for t, (name, w) in enumerate(MIXTURES.items()):
        w = mixture_pmf(w)
        labels_ok(np.concatenate(out[t * OPS:(t + 1) * OPS]).ravel(), w, f"mixture of {name} components")


def hypothesis_pmf(multihypo, sfidx):
    """the Categorical that mhidx is drawn from, restated from ExplicitDiscreteMarginalizations.jl:161-186: values 0 .. nvars
    (0 = the bad-init null hypothesis, i = fractional variable i, 1-based).  Solve-for variable certain: p = multihypo itself;
    fractional: a null hypothesis of weight 1 / (nunc + 1) is prepended and the rest scaled by nunc / (nunc + 1)."""
    p = np.asarray(multihypo, dtype=float)
    nunc = int((p > 0).sum())
    if p[sfidx] == 0.0:
        return np.concatenate([[0.0], p])
    full = np.concatenate([[1.0 / (nunc + 1)], nunc / (nunc + 1.0) * p])
    return full / full.sum()


def case_hypothesis_selection(backend):
    """mhidx_out from the side buffer: nullhypo = 0.1, 0.5, 0.9 on a prior (0 = null, 1 = the factor), and multihypo with 2
    and 3 fractional variables on a LinearRelative, solving for the certain and for a fractional variable"""
    ops = 600  # 307 200 draws per recipe
    descs, want = [], []
    for t, nh in enumerate((0.1, 0.5, 0.9)):
        descs += [prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [1.0], 0)], nullhypo=nh) for s in pool_seeds(50 + t, ops)]
        want.append((f"nullhypo = {nh}", np.array([nh, 1.0 - nh])))
    t = 3
    for mh in ([0.0, 0.3, 0.7], [0.0, 0.2, 0.3, 0.5]):
        for sf in (0, 1):
            for s in pool_seeds(50 + t, ops):
                d = prior_desc(abi.EUCLID1, s, [(1.0, [0.5], [0.1], 0)], kind=abi.F_LINREL)
                d.nvars, d.sfidx, d.has_multihypo, d.inflate_cycles = len(mh), sf, 1, 1
                for i, p in enumerate(mh):
                    d.multihypo[i], d.var_slot[i] = p, 1 + i
                descs.append(d)
            want.append((f"multihypo = {mh}, solving for variable {sf}", hypothesis_pmf(mh, sf)))
            t += 1
    for i, d in enumerate(descs):
        d.mhidx_out = i * NP
    rng = np.random.default_rng(5)

    def setup(be):
        for v in range(4):
            be.slot_write(1 + v, abi.EUCLID1, rng.normal(v, 0.5, (NP, 1)), np.ones(1))
    _, side = run_pool(backend, NP, descs, n_in=5, setup=setup, side_ints=len(descs) * NP)
    for t, (name, p) in enumerate(want):
        mh = side[t * ops * NP:(t + 1) * ops * NP]
        assert mh.min() >= 0 and mh.max() < p.size, name
        chi2_ok(np.bincount(mh, minlength=p.size), p, name)


# ---- entropy of null particles ---------------------------------------------------------------------------------------------------
def running_geodesic_mean(x, circ):
    """mean(M, pts, GeodesicInterpolation()) of one coordinate (Manifolds.jl; services/VariableStatistics.jl:30): the running
    mean m_i = m_{i-1} + log_{m_{i-1}}(x_i) / i, the step and the mean wrapped to [-pi, pi) on a circular coordinate"""
    m = float(x[0])
    for i in range(1, x.size):
        dl = x[i] - m
        if circ:
            dl = (dl + np.pi) % (2 * np.pi) - np.pi
        m += dl / (i + 1)
        if circ:
            m = (m + np.pi) % (2 * np.pi) - np.pi
    return m


def std_basic_spread(manifold, c):
    """calcStdBasicSpread (services/VariableStatistics.jl:22-36): sigma = sqrt(sum_i d(mu, x_i)^2 / (N - 1)) about the running
    geodesic mean, 1.0 below 1e-10.  d^2 on SE(2) = |dt|^2 + |log(R_mu' R_i)|_F^2 = |dt|^2 + 2 dtheta^2 (the Frobenius norm of
    the skew matrix of dtheta)."""
    acc = np.zeros(c.shape[0])
    for d in range(c.shape[1]):
        circ = (manifold == abi.CIRCULAR) or (manifold == abi.SE2 and d == 2)
        dl = c[:, d] - running_geodesic_mean(c[:, d], circ)
        acc += (2.0 if manifold == abi.SE2 and circ else 1.0) * wrap(dl) ** 2 if circ else dl ** 2
    sg = np.sqrt(acc.sum() / (c.shape[0] - 1))
    return sg if sg > 1e-10 else 1.0


def entropy_shapes(manifold, N):
    rng = np.random.default_rng(60 + manifold)
    D = abi.MANIFOLD_DIM[manifold]
    if manifold == abi.CIRCULAR:  # the shapes of test_gpu_device_math.py: one mode, straddling the seam, four doors
        return {"one mode": rng.normal(0.4, 0.3, (N, 1)), "near pi": wrap(rng.normal(3.1, 0.4, (N, 1))),
                "doors": wrap(rng.choice([-2.5, -0.8, 0.9, 2.6], (N, 1)) + rng.normal(0, 0.1, (N, 1)))}
    if manifold == abi.SE2:
        a = np.concatenate([rng.normal(0, 1.0, (N, 2)), wrap(rng.normal(3.1, 0.3, (N, 1)))], axis=1)
        b = np.concatenate([rng.normal([5.0, -3.0], [0.5, 1.5], (N, 2)), rng.normal(-1.0, 0.2, (N, 1))], axis=1)
        return {"heading near pi": a, "one mode": b}
    two = np.where(rng.uniform(size=(N, 1)) < 0.3, -4.0, 3.0) + rng.normal(0, 0.5, (N, D))
    return {"one mode": rng.normal(1.0, 2.0, (N, D)), "two modes": two}


def case_entropy_of_null_particles(backend, manifold):
    """Prior with nullhypo = 0.5 over a belief held in slot 0: particles whose mhidx says null keep their value plus
    spreadNH * spread * (u - 1/2) per coordinate (addEntropyOnManifold!, EvalFactor.jl:95-132,464-476) -- so
    (out - old) / (spreadNH * spread) is U(-1/2, 1/2); the others are the prior's own draw.  `spread` is computed HERE from the
    reference's definition, not by the checker."""
    mu, L, circ = GAUSS[manifold]
    D = abi.MANIFOLD_DIM[manifold]
    for name, old in entropy_shapes(manifold, NP).items():
        spread = 3.0 * std_basic_spread(manifold, old)
        descs = [prior_desc(manifold, s, [(1.0, mu, L, 0)], nullhypo=0.5) for s in pool_seeds(70 + manifold, OPS)]
        for i, d in enumerate(descs):
            d.mhidx_out = i * NP
        out, side = run_pool(backend, NP, descs, setup=lambda be: be.slot_write(0, manifold, to_points(manifold, old), np.ones(D)),
                             side_ints=OPS * NP)
        x, null = np.concatenate(out), side == 0
        assert ((side == 0) | (side == 1)).all()
        e = x[null] - np.tile(old, (OPS, 1))[null]
        for d in circ:
            e[:, d] = wrap(e[:, d])  # the widths used here stay below 2 pi
        assert not circ or spread < 2 * np.pi, spread
        unit_entropy_ok(e / spread, f"entropy on manifold {manifold}, {name}")
        chi2_ok([null.sum(), (~null).sum()], [0.5, 0.5], f"null fraction on manifold {manifold}, {name}")
        gaussian_ok(x[~null], mu, L, f"non-null particles on manifold {manifold}, {name}", circ)


# ---- draws from a belief ---------------------------------------------------------------------------------------------------------
BW = {abi.EUCLID1: [0.01], abi.EUCLID2: [0.02, 0.005], abi.EUCLID3: [0.01, 0.02, 0.005], abi.CIRCULAR: [0.0002],
      abi.SE2: [0.01, 0.02, 0.0002]}
_ARC0, _ARC = 3.0, 0.012  # circular lattice: from 3.0 on, across the seam at pi, 60 bandwidths apart (512 points: 6.14 < 2 pi)


def lattice(manifold, cd):
    """cd source points at least 50 bandwidths apart on every coordinate (Euclidean coordinate d: spacing 1 + d >= 50 bw;
    circular: 0.012 = 60 bw): an output names its kernel"""
    i = np.arange(cd, dtype=float)
    c = np.stack([(1.0 + d) * i for d in range(abi.MANIFOLD_DIM[manifold])], axis=1)
    if manifold in (abi.CIRCULAR, abi.SE2):
        c[:, -1] = wrap(_ARC0 + _ARC * i)
    return c


def nearest_kernel(manifold, x):
    if manifold == abi.CIRCULAR:
        return np.floor(((wrap(x[:, 0] - _ARC0) + _ARC / 2) % (2 * np.pi)) / _ARC).astype(int)
    return np.rint(x[:, 0]).astype(int)


def kernel_residuals(x, manifold, src, what):
    """x: draws of `random kernel + bw * randn` from the density (src, BW).  -> (kernel index, residual in bandwidths): the
    nearest lattice point is the kernel (the next one is >= 50 bandwidths away: a residual beyond 8 has probability
    2 Phi(-8) = 1.2e-15 per draw -- asserted), wrapped on circular coordinates"""
    idx = nearest_kernel(manifold, x)
    assert idx.min() >= 0 and idx.max() < src.shape[0], f"{what}: kernel index out of the density's {src.shape[0]} points"
    r = x - src[idx]
    if manifold in (abi.CIRCULAR, abi.SE2):
        r[:, -1] = wrap(r[:, -1])
    w = r / np.asarray(BW[manifold])
    assert np.abs(w).max() < 8.0, f"{what}: a residual of {np.abs(w).max():.1f} bandwidths"
    return idx, w


def kernel_noise_ok(w, what):
    """w (n, D): residuals in bandwidths, pooled over the densities of a case: N(0, 1) per coordinate (KS; variance with s.e.
    sqrt(2 / n)), coordinates independent"""
    q = stats.norm.cdf(w)
    for d in range(w.shape[1]):
        ks_ok(w[:, d], stats.norm.cdf, f"{what}: kernel noise, coordinate {d}")
        z_ok(float((np.mean(w[:, d] ** 2) - 1.0) / np.sqrt(2.0 / w.shape[0])), f"{what}: kernel noise variance, coordinate {d}")
        for e in range(d):
            independent_uniforms_ok(q[:, d], q[:, e], f"{what}: kernel noise, coordinates ({e},{d})")


def belief_draws_ok(per_cd, manifold, what):
    """per_cd: [(source lattice, draws)] -- kernel counts per density, the noise pooled over them"""
    ws = []
    for src, x in per_cd:
        idx, w = kernel_residuals(x, manifold, src, f"{what}, cd = {src.shape[0]}")
        kernel_pick_ok(idx, src.shape[0], f"{what}, cd = {src.shape[0]}")
        ws.append(w)
    kernel_noise_ok(np.concatenate(ws), what)


BELIEF_OPS = 400  # proposals per density: 204 800 picks each; the pooled noise of a case has >= 5.7e5 draws (power checks)
COUNTS = (1, 2, 100, NP - 1, NP)  # cd: both ends, a mid value


def case_msgprior_draw(backend, manifold):
    """MsgPrior{MKD}: sample(belief, 1) = random kernel + bw * randn under PURP_KDESEL / PURP_KDENOISE"""
    ops = BELIEF_OPS
    srcs = [lattice(manifold, cd) for cd in COUNTS]
    descs = []
    for t in range(len(COUNTS)):
        descs += [prior_desc(manifold, s, [(1.0, [0.0], [1.0], 0)], kind=abi.F_MSGPRIOR, msg_slot=1 + t) for s in pool_seeds(80 + 8 * manifold + t, ops)]

    def setup(be):
        for t, c in enumerate(srcs):
            be.belief_write(1 + t, manifold, to_points(manifold, c), BW[manifold])
    out, _ = run_pool(backend, NP, descs, n_in=1 + len(COUNTS), setup=setup)
    belief_draws_ok([(srcs[t], np.concatenate(out[t * ops:(t + 1) * ops])) for t in range(len(COUNTS))], manifold,
                    f"MsgPrior draw, manifold {manifold}")


def case_passthrough_topup(backend, manifold):
    """PartialPriorPassThrough with keep_count = 2 (graph initialisation, GraphInit.jl:174-177): the first cd outputs ARE the
    density's points, the rest are draws from its KDE under PURP_OLDSEL / PURP_OLDNOISE"""
    ops = BELIEF_OPS
    counts = [cd for cd in COUNTS if cd < NP]
    srcs = [lattice(manifold, cd) for cd in counts]
    descs = []
    for t in range(len(counts)):
        for s in pool_seeds(120 + 8 * manifold + t, ops):
            d = prior_desc(manifold, s, [(1.0, [0.0], [1.0], 0)], kind=abi.F_PASSTHROUGH, msg_slot=1 + t)
            d.keep_count = 2
            descs.append(d)

    def setup(be):
        for t, c in enumerate(srcs):
            be.belief_write(1 + t, manifold, to_points(manifold, c), BW[manifold])
    out, _ = run_pool(backend, NP, descs, n_in=1 + len(counts), setup=setup)
    per_cd = []
    for t, cd in enumerate(counts):
        o = out[t * ops:(t + 1) * ops]
        for x in o:
            dl = x[:cd] - srcs[t]
            if manifold in (abi.CIRCULAR, abi.SE2):
                dl[:, -1] = wrap(dl[:, -1])
            assert np.abs(dl).max() < 1e-12, f"keep_count = 2, manifold {manifold}, cd = {cd}: the density's own points moved"
        per_cd.append((srcs[t], np.concatenate([x[cd:] for x in o])))
    belief_draws_ok(per_cd, manifold, f"keep_count = 2, manifold {manifold}")


def case_resample(backend, manifold):
    """nbp_run_resample: beliefs with fewer than N points topped up in place with draws from their own KDE"""
    ops = BELIEF_OPS
    counts = [cd for cd in COUNTS if cd < NP]
    be = backend(NP, len(counts) * ops, 0)
    try:
        for t, cd in enumerate(counts):
            for i in range(ops):
                be.belief_write(t * ops + i, manifold, to_points(manifold, lattice(manifold, cd)), BW[manifold])
        be.run_resample(list(range(len(counts) * ops)), [manifold] * (len(counts) * ops), seed=SEED0 + 777)
        out = [coords(manifold, be.slot_read(s, manifold)[0]) for s in range(len(counts) * ops)]
    finally:
        be.close()
    per_cd = []
    for t, cd in enumerate(counts):
        o, src = out[t * ops:(t + 1) * ops], lattice(manifold, cd)
        for x in o:
            dl = x[:cd] - src
            if manifold in (abi.CIRCULAR, abi.SE2):
                dl[:, -1] = wrap(dl[:, -1])
            assert np.abs(dl).max() < 1e-12, f"resample, manifold {manifold}, cd = {cd}: the belief's own points moved"
        per_cd.append((src, np.concatenate([x[cd:] for x in o])))
    belief_draws_ok(per_cd, manifold, f"resample, manifold {manifold}")


def case_kde_measurement_and_anyn(backend):
    """LinearRelative whose measurement is a KDE (meas_kde), solved forward from an operand with FEWER points: x1 = x0[j] + z,
    z = kernel i of the measurement density + bw * randn, j = n for n < c0 and uniform over c0 beyond (_getindex_anyn,
    NumericalCalculations.jl:377-381).  x0 sits on a lattice of spacing 1000, the kernels on one of spacing 1 (100
    bandwidths): the output names both.  The per-particle search ends within 1e-6 of the root (2-norm residual tolerance),
    1e-4 bandwidths: invisible to a KS of 10^5 draws (4e-5 in CDF against a threshold of ~5e-3)."""
    ops, c0 = BELIEF_OPS, 5
    per_cd = []
    for cd in COUNTS:
        src = lattice(abi.EUCLID1, cd)
        descs = []
        for s in pool_seeds(200 + cd, ops):
            d = prior_desc(abi.EUCLID1, s, [(1.0, [0.0], [1.0], 0)], kind=abi.F_LINREL)
            d.nvars, d.sfidx, d.meas_kde, d.inflate_cycles = 2, 1, 3, 1
            d.var_slot[0], d.var_slot[1] = 1, 0
            descs.append(d)

        def setup(be):
            be.belief_write(1, abi.EUCLID1, 1000.0 * np.arange(c0).reshape(-1, 1), np.ones(1))
            be.belief_write(2, abi.EUCLID1, src, BW[abi.EUCLID1])
        out, _ = run_pool(backend, NP, descs, n_in=3, setup=setup)
        x = np.concatenate(out).ravel()
        j = np.floor((x + 10.0) / 1000.0).astype(int)
        assert j.min() >= 0 and j.max() < c0
        n = np.tile(np.arange(NP), ops)
        assert (j[n < c0] == n[n < c0]).all(), "particles within the operand's count read their own element"
        kernel_pick_ok(j[n >= c0], c0, f"anyn index over {c0} points (cd = {cd})")
        per_cd.append((src, (x - 1000.0 * j).reshape(-1, 1)))
    belief_draws_ok(per_cd, abi.EUCLID1, "KDE measurement")


# ---- independence across what the counters separate ------------------------------------------------------------------------------
def case_independence(backend):
    ops = OPS
    base = SEED0 + (999 << 40)
    seeds = [base + 2 * i for i in range(ops)]  # s, s + 2, ...: s + 1 and s + 2^32 are run beside them
    uni = [(1.0, [0.0], [1.0], abi.DIST_UNIFORM)]
    descs = [prior_desc(abi.EUCLID1, s, uni) for s in seeds]
    descs += [prior_desc(abi.EUCLID1, s + 1, uni) for s in seeds]
    descs += [prior_desc(abi.EUCLID1, (s + 2 ** 32) & (2 ** 64 - 1), uni) for s in seeds]
    descs += [prior_desc(abi.EUCLID2, s, [(1.0, [0.0, 0.0], [1.0, 1.0], 0)]) for s in seeds]
    ent = [prior_desc(abi.EUCLID1, s, uni, mhidx_in=0) for s in seeds]  # injected mhidx = 0: every particle takes entropy
    out, _ = run_pool(backend, NP, descs + ent, side_ints=NP, side_init=np.zeros(NP, dtype=np.int32))
    u = np.stack([o.ravel() for o in out[:ops]])
    u1 = np.stack([o.ravel() for o in out[ops:2 * ops]])
    u32 = np.stack([o.ravel() for o in out[2 * ops:3 * ops]])
    g = np.concatenate(out[3 * ops:4 * ops])
    # slot 0 holds zeros: spread = 1 (the 1e-10 floor), spreadNH = 3 -> out = 3 (u_entropy - 1/2)
    e = np.stack([o.ravel() for o in out[4 * ops:]]) / 3.0 + 0.5
    independent_uniforms_ok(u[:, :-1].ravel(), u[:, 1:].ravel(), "particles n and n + 1 of one op")
    independent_uniforms_ok(u.ravel(), u1.ravel(), "one particle under seeds s and s + 1")
    independent_uniforms_ok(u.ravel(), u32.ravel(), "one particle under seeds s and s + 2^32")
    ua, ub = np.exp(-0.5 * (g ** 2).sum(axis=1)), (np.arctan2(g[:, 1], g[:, 0]) / (2 * np.pi)) % 1.0
    ks_ok(ua, lambda t: t, "ua recovered from the normal pair")
    ks_ok(ub, lambda t: t, "ub recovered from the normal pair")
    independent_uniforms_ok(ua, ub, "ua and ub of one block")
    ks_ok(e.ravel(), lambda t: t, "entropy uniform of an all-null op")
    independent_uniforms_ok(u.ravel(), e.ravel(), "measurement and entropy of one op")
