"""Shared cases of the credible-region tests (tests/test_credible.py on the CPU, tests/test_gpu_credible.py on the device): the
clouds (those of ppe_cases through stats_cases), the items, the queries, and the criteria a result is held to.

The criteria (derived, not measured; the definition is DESIGN.md 3, "Credible regions" / incrementalinference.jl_amd/credible.py):

  logdens, l_q  |dev - ref| <= 1e-12 (1 + |ref|) against credible_numpy on the belief read back.  The bound stats_cases derives for
              the kld's log densities, for the same reasons -- the same device functions are at work: exp_nonpos carries ~3e-15
              relative error, a sum of <= 512 positive terms 512 * 2^-53 ~ 6e-14, nbpm_log one ulp, the exponent e_ij a few ulps of
              itself (it enters M at full size: hence the term relative to |l|); 1e-12 is an order of magnitude above these together.
              credible_numpy forms e_ij by the device's own operations and adds exactly (math.fsum).
  order       np.lexsort((arange(c), logdens_dev)) exactly: a sort of the device's OWN values has one right answer.
  levels      log_level[a] is logdens_dev[order[c - k]], k = ceil(a c) clamped, bit for bit; n_inside = #{logdens_dev >= level} and
              n_above = #{logdens_dev > l_q_dev} exactly; mass = n_above / c bit for bit; log_min / log_max the ends of the order.
  conditions  of the comparison of those integers and levels with NUMPY's, not measurements: the restatement's l_i and l_q differ from
              the device's by up to the bound, so a count can differ where two values lie closer than that.  Asserted first:
              no |l_i - l_q| and no gap l[(c - k)] - l[(c - k) - 1] of the ascending order lies below 2 x the bound -- but for a gap
              of exactly 0.0, which no seed avoids: two points tie ((x_0 - x_1)^2 = (x_1 - x_0)^2 makes l_0 and l_1 the same bits
              -- unless the pair straddles +-pi on a circular coordinate, where the two wraps round differently: such a pair is
              a near-tie and the seeds avoid it), so do two mutual nearest neighbours whose other terms vanish beside 1.0 (three
              points, two of them close), and all-identical clouds.  Where the restatement ties exactly the DEVICE'S two values
              must be the same bits too (asserted), and the counts then agree as they do elsewhere.  `exact_ties` names the
              beliefs that tie as a whole (identical clouds): their l_i are held to be all equal, and an own point as a query,
              whose l_q equals the l_i in exact arithmetic only, is not counted against numpy.  Then stats_cases' wrap condition -- no
              |x - mean|, no |x_i - x_j|, no |q - x_j| and no |mean + Q| on a circular coordinate within 1e-9 of pi, where the wrap's
              branch could differ.  tests/test_credible.py asserts on the CPU that the seeds used meet them.
  quantiles   Euclidean and circle coordinates: the bits of the hand-written type-7 formula on the coordinates read back, about
              the device's mean (the same subtraction, wrap, sort of distinct-or-equal values, two differences, one product, one
              sum).  The SE(2) heading comes back through cos / sin and atan2, an ulp of theta per point (4.4e-16 at |theta| <= pi)
              and of the mean: a quantile is a convex combination of two order statistics, each moved by at most that, plus the
              wrap about the mean: |dev - ref| <= 4e-15, stats_cases' allowance for the same round trip.
  mean        the bits of run_ppe's mean of the same slots.

Calibration of the DEFINITION (tests/test_credible.py; no device involved): Euclid(3) standard-normal clouds of N = 200 with the
rule-of-thumb bandwidth h_d = std_d (4 / ((D + 2) N))^(1 / (D + 4)), the truth drawn from the same law, T = 2000 trials at seed
CAL_SEED.  |coverage(a) - a| <= 3.89 sqrt(a (1 - a) / T) + b_a, 3.89 the two-sided 1e-4 normal quantile (the project's false-alarm
budget) and b_a = CAL_BIAS[a] the bias of the definition itself, measured ONCE as |coverage - a| over 20 000 trials at another seed
(CAL_BIAS_SEED) by

    python -c "import sys; sys.path.insert(0, 'tests'); import credible_cases as cc; print(cc.calibration(20000, cc.CAL_BIAS_SEED))"

which printed  ({0.5: 0.50625, 0.95: 0.9516}, {0.5: 0.42765, 0.95: 0.8492})  -- leave-one-out, then the self term in -- after two
minutes on one core: b_0.5 = 0.00625, b_0.95 = 0.0016.  At T = 2000 the bounds are 0.0497 and 0.0206.  The self-term-in variant
misses 0.95 by 0.10, five of the bound's widths and twenty standard deviations of the binomial term: the same test shows that it
fails (at 0.5 it misses by 0.07, which the test prints and does not assert: 1.5 widths).
"""
import math

import numpy as np

import ppe_cases as pc
import stats_cases as sc
from parity_utils import abi, coords, iif

cr = iif.credible
MANIFOLDS = pc.MANIFOLDS
MASS = (0.5, 0.9, 0.95, 1.0, 1e-9)
PROBS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)
L_RTOL = 1e-12
WRAP_MARGIN = sc.WRAP_MARGIN
HEADING_ATOL = 4e-15
FULL_COUNTS = (64, 65, 200, 257, 512)                     # every manifold and cloud at full count: seed 400 + N
BELOW_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 150)  # counts below the context size at N = 200: seed 18
BELOW_CLOUDS = ("gaussian", "across_pi", "identical")
MASK_SEED, BATCH_SEED, BATCH_CLOUD_SEED, MANY_SEED = 27, 37, 77, 47
CAL_SEED, CAL_BIAS_SEED, CAL_T = 20261020, 777, 2000
CAL_BIAS = {0.5: 0.00625, 0.95: 0.0016}


def full_items(N):
    return [(m, kind, N) for m in MANIFOLDS for kind in pc.CLOUDS]


def below_items():
    return [(m, kind, c) for m in MANIFOLDS for c in BELOW_COUNTS for kind in BELOW_CLOUDS]


def mask_items(N):
    """every non-empty coordinate mask of every manifold -> ([(manifold, kind, count)], masks)"""
    items, masks = [], []
    for m in MANIFOLDS:
        for k in range(1, 1 << abi.MANIFOLD_DIM[m]):
            items.append((m, ("gaussian", "two_cluster", "across_pi")[k % 3], N))
            masks.append(k)
    return items, masks


def batch_items(n, N, seed):
    """mixed manifolds, clouds, counts and masks -> (items, masks, number of queries per belief: some 0)"""
    rng = np.random.default_rng(seed)
    items, masks, nq = [], [], []
    for _ in range(n):
        m = MANIFOLDS[rng.integers(5)]
        items.append((m, pc.CLOUDS[rng.integers(5)], int(rng.choice([N, N, N, 150, 129, 63, 3, 2, 1]))))
        masks.append(int(rng.integers(1, 1 << abi.MANIFOLD_DIM[m])))
        nq.append(int(rng.choice([0, 0, 1, 3, 7])))
    return items, masks, nq


def full_mask(manifold):
    return (1 << abi.MANIFOLD_DIM[manifold]) - 1


def queries_for(manifold, X, bw, rng, n=4):
    """n reference points in tangent coordinates (n x 3, entries beyond D zero): points about the cloud; from n = 2 on the first
    is the belief's own point 0 and the last lies 1e3 bandwidths from point 0 on every Euclidean coordinate (3 rad on a circular
    one)"""
    D = abi.MANIFOLD_DIM[manifold]
    Q = np.zeros((n, abi.MAXD))
    for k in range(n):
        Q[k, :D] = X[rng.integers(len(X))] + rng.normal(0, 0.3, D)
    if n >= 2:
        Q[0, :D] = X[0]
        Q[n - 1, :D] = X[0] + 1e3 * np.asarray(bw)[:D]
        for d in pc.circular_coords(manifold):
            Q[n - 1, d] = X[0, d] + 3.0
    for d in pc.circular_coords(manifold):
        Q[:, d] = pc.wrap(Q[:, d])
    return Q


def scenario(name):
    """the beliefs of one device test -> (N, items, masks, queries per belief, seed); tests/test_credible.py walks them all on the
    CPU and asserts the conditions of the comparison"""
    if name.startswith("full"):
        N = int(name[4:])
        items = full_items(N)
        return N, items, [full_mask(m) for m, _, _ in items], [4] * len(items), 400 + N
    if name == "below":
        items = below_items()
        return 200, items, [full_mask(m) for m, _, _ in items], [4] * len(items), 18
    if name == "masks":
        items, masks = mask_items(200)
        return 200, items, masks, [4] * len(items), MASK_SEED
    if name == "batch":
        items, masks, nq = batch_items(300, 200, BATCH_SEED)
        return 200, items, masks, nq, BATCH_CLOUD_SEED
    raise KeyError(name)


SCENARIOS = tuple(f"full{N}" for N in FULL_COUNTS) + ("below", "masks", "batch")


def beliefs(items, nq, seed):
    """-> per item (tangent coordinates X, the hand bandwidth, queries q x 3), drawn in order from two generators"""
    Xs = sc.clouds(items, seed)
    rng = np.random.default_rng(seed + 1000)
    return [(X, pc.hand_bandwidth(m), queries_for(m, X, pc.hand_bandwidth(m), rng, n)) for (m, _, _), X, n in zip(items, Xs, nq)]


def exact_ties(kind, c):
    """the beliefs whose l_i tie exactly, on the device and in numpy alike"""
    return kind == "identical"


# ---- the conditions ----------------------------------------------------------------------------------------------------------
def l_bound(l):
    return L_RTOL * (1.0 + np.abs(l))


def conditions(manifold, mask, X, mean, ref, Q, mass, ties=False):
    """the conditions of the comparison with numpy's counts and levels -> the worst ratio (value / what it must exceed), > 1 when
    all hold; ref: credible_numpy's result on X.  ties: an all-identical cloud, whose equal l are exact on both sides"""
    D, c = abi.MANIFOLD_DIM[manifold], X.shape[0]
    worst = np.inf
    if c >= 2 and np.isfinite(ref.logdens).all() and not ties:
        ls = ref.logdens[ref.order]
        for a in mass:
            p = c - cr.level_rank(a, c)
            if p > 0 and ls[p] != ls[p - 1]:  # (an exact tie: check_belief holds the device to it)
                worst = min(worst, (ls[p] - ls[p - 1]) / (2 * l_bound(ls[p])))
        for lq in ref.q_logdens:
            worst = min(worst, float((np.abs(ref.logdens - lq) / (2 * l_bound(lq))).min()))
    margin = min(sc.belief_wrap_margin(manifold, X, mean), sc.pair_wrap_margin(manifold, X, X))
    for d in pc.circular_coords(manifold):
        if Q is not None and len(Q) and (mask >> d & 1):
            margin = min(margin, float(np.abs(np.abs(Q[:, d, None] - X[None, :, d]) - np.pi).min()))
        if ref.quantiles.shape[1]:  # (mean + Q lies within 1e-9 of +-pi exactly when its wrapped value does)
            margin = min(margin, float(np.abs(np.abs(ref.quantiles[d]) - np.pi).min()))
    return min(worst, margin / WRAP_MARGIN)


# ---- the criteria --------------------------------------------------------------------------------------------------------------
def check_belief(manifold, mask, pts, bw, mass, probs, rec, logdens, order, Q=None, qrecs=None, what="", ties=False):
    """one belief of a run_credible against the criteria: pts / bw the belief as read back (host form), rec its record, logdens /
    order its rows (N entries), Q / qrecs its queries (q x 3) and their records -> the worst |dev - ref| / bound"""
    D, X = abi.MANIFOLD_DIM[manifold], coords(manifold, np.asarray(pts))
    c, N, nm, npr = X.shape[0], len(logdens), len(mass), len(probs)
    assert rec["count"] == c and rec["pad"] == 0, (what, rec["count"], c)
    assert np.all(rec["log_level"][nm:] == 0) and np.all(rec["n_inside"][nm:] == 0) and np.all(rec["mean"][D:] == 0), (what, rec)
    assert np.all(rec["quant"][D:] == 0) and np.all(rec["quant"][:, npr:] == 0), (what, rec["quant"])
    assert np.isnan(logdens[c:]).all() and np.all(order[c:] == -1), (what, logdens[c:], order[c:])
    mean = rec["mean"]
    valid = all(np.isfinite(bw[d]) and bw[d] > 0 for d in range(D) if mask >> d & 1)
    Qd = None if Q is None else np.asarray(Q)[:, :D]
    ref = cr.credible_numpy(manifold, pts, bw, mask, mass, probs, Qd, mean=mean[:D])
    worst = 0.0
    ld, od = logdens[:c], order[:c]
    if not valid or c < 2:
        assert np.isnan(ld).all() and np.isnan(rec["log_level"][:nm]).all() and np.all(rec["n_inside"] == 0), (what, ld, rec)
        assert np.isnan(rec["log_min"]) and np.isnan(rec["log_max"]), (what, rec)
        assert np.array_equal(od, np.arange(c) if valid else np.full(c, -1)), (what, od)
        if qrecs is not None and len(qrecs):
            assert np.isnan(qrecs["mass"]).all() and np.all(qrecs["n_above"] == -1), (what, qrecs)
            if valid:  # (c == 1: the density of the one kernel stands)
                assert np.all(np.abs(qrecs["logdens"] - ref.q_logdens) <= l_bound(ref.q_logdens)), (what, qrecs["logdens"], ref.q_logdens)
            else:
                assert np.isnan(qrecs["logdens"]).all(), (what, qrecs)
    else:
        cond = conditions(manifold, mask, X, mean[:D], ref, Qd, mass, ties)
        assert cond > 1.0, (what, "conditions of the comparison", cond)
        err = np.abs(ld - ref.logdens) / l_bound(ref.logdens)
        worst = float(err.max())
        assert np.isfinite(ld).all() and worst <= 1.0, (what, "logdens", worst, int(err.argmax()))
        assert np.array_equal(od, np.lexsort((np.arange(c), ld))), (what, "order")
        if ties:  # an all-identical cloud: every l the same bits, the order by index, every region the whole belief
            assert np.all(ld == ld[0]) and np.array_equal(od, np.arange(c)) and np.all(rec["n_inside"][:nm] == c), (what, "ties")
        for a in range(nm):
            k = cr.level_rank(mass[a], c)
            lev = rec["log_level"][a]
            assert lev.tobytes() == ld[od[c - k]].tobytes(), (what, "level", a, lev, ld[od[c - k]])
            if k < c and ref.logdens[ref.order[c - k]] == ref.logdens[ref.order[c - k - 1]]:  # the restatement ties here: so must the device
                assert ld[od[c - k]] == ld[od[c - k - 1]], (what, "tie at the level boundary", a, ld[od[c - k]], ld[od[c - k - 1]])
            assert rec["n_inside"][a] == int((ld >= lev).sum()) >= k, (what, "n_inside", a, rec["n_inside"][a], k)
            assert abs(lev - ref.log_levels[a]) <= l_bound(ref.log_levels[a]), (what, "level against numpy", a, lev, ref.log_levels[a])
            assert ties or rec["n_inside"][a] == ref.n_inside[a], (what, "n_inside against numpy", a, rec["n_inside"][a], ref.n_inside[a])
        assert rec["log_min"].tobytes() == ld[od[0]].tobytes() and rec["log_max"].tobytes() == ld[od[-1]].tobytes(), (what, rec)
        if qrecs is not None and len(qrecs):
            qerr = np.abs(qrecs["logdens"] - ref.q_logdens) / l_bound(ref.q_logdens)
            worst = max(worst, float(qerr.max()))
            assert np.isfinite(qrecs["logdens"]).all() and qerr.max() <= 1.0, (what, "l_q", qerr.max())
            for j in range(len(qrecs)):
                above = int((ld > qrecs["logdens"][j]).sum())
                assert qrecs["n_above"][j] == above, (what, "n_above", j, qrecs["n_above"][j], above)
                assert ties or above == ref.q_n_above[j], (what, "n_above against numpy", j, above, ref.q_n_above[j])
                assert qrecs["mass"][j].tobytes() == np.float64(above / c).tobytes() and qrecs["pad"][j] == 0, (what, "mass", j)
    # the quantiles stand whatever the bandwidth
    for d in range(D):
        got, want = rec["quant"][d, :npr], ref.quantiles[d]
        if manifold == abi.SE2 and d == 2:
            assert np.abs(pc.wrap(got - want)).max() <= HEADING_ATOL, (what, "heading quantiles", got, want)
        else:
            assert got.tobytes() == want.tobytes(), (what, "quantiles", d, got, want, got - want)
    return worst


# ---- calibration of the definition ------------------------------------------------------------------------------------------------
def rule_of_thumb(X):
    n, D = X.shape
    return X.std(axis=0, ddof=1) * (4.0 / ((D + 2) * n)) ** (1.0 / (D + 4))


def calibration(T, seed, D=3, N=200, at=(0.5, 0.95)):
    """coverage of a truth drawn from the clouds' own law at the masses `at`, over T trials -> (leave-one-out {a: coverage}, the
    same with the self term in): the restatement's functions, the masses formed as credible_numpy forms them"""
    man = (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3)[D - 1]
    rng = np.random.default_rng(seed)
    loo, own = np.zeros(T), np.zeros(T)
    for t in range(T):
        X, q = rng.normal(size=(N, D)), rng.normal(size=(1, D))
        bw = rule_of_thumb(X)
        lq = cr.log_density_numpy(man, X, bw, full_mask(man), q)[0]
        loo[t] = float((cr.log_density_loo_numpy(man, X, bw, full_mask(man)) > lq).sum()) / float(N)
        own[t] = float((cr.log_density_loo_numpy(man, X, bw, full_mask(man), self_term=True) > lq).sum()) / float(N)
    return ({a: float(v) for a, v in zip(at, cr.coverage(loo, at))}, {a: float(v) for a, v in zip(at, cr.coverage(own, at))})


def calibration_bound(a, T):
    return 3.89 * math.sqrt(a * (1.0 - a) / T) + CAL_BIAS[a]
