"""CPU: the known answers of tests/sampling_cases.py on the oracle (the same cases run on the GPU in
tests/test_gpu_sampling_known_answers.py), the Philox4x32-10 of the test module against Random123's published vectors, and
the power checks: every statistic of sampling_cases.py is fed a numpy sample of the size the backend cases use, drawn from a
slightly wrong law, and its threshold has to reject it (and to accept the right law: a statistic that rejects everything
has no teeth either)."""
import numpy as np
import pytest

import sampling_cases as sc
from parity_utils import abi

MANIFOLDS = [abi.EUCLID1, abi.EUCLID2, abi.EUCLID3, abi.CIRCULAR, abi.SE2]
BELIEF_MANIFOLDS = [abi.EUCLID1, abi.EUCLID2, abi.CIRCULAR, abi.SE2]


def test_philox_known_answer_vectors():
    sc.case_philox_known_answers()


@pytest.mark.parametrize("N", sc.STREAM_N)
def test_stream_is_philox(oracle_backend, N):
    assert sc.case_stream_is_philox(oracle_backend, N) == "ran"  # the checker takes every N


@pytest.mark.parametrize("manifold", MANIFOLDS)
def test_gaussian_measurement(oracle_backend, manifold):
    sc.case_gaussian_measurement(oracle_backend, manifold)


def test_uniform_and_rayleigh(oracle_backend):
    sc.case_uniform_and_rayleigh(oracle_backend)


def test_tabulated(oracle_backend):
    sc.case_tabulated(oracle_backend)


def test_mixture_labels(oracle_backend):
    sc.case_mixture_labels(oracle_backend)


def test_hypothesis_selection(oracle_backend):
    sc.case_hypothesis_selection(oracle_backend)


@pytest.mark.parametrize("manifold", MANIFOLDS)
def test_entropy_of_null_particles(oracle_backend, manifold):
    sc.case_entropy_of_null_particles(oracle_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_msgprior_draw(oracle_backend, manifold):
    sc.case_msgprior_draw(oracle_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_passthrough_topup(oracle_backend, manifold):
    sc.case_passthrough_topup(oracle_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_resample(oracle_backend, manifold):
    sc.case_resample(oracle_backend, manifold)


def test_kde_measurement_and_anyn(oracle_backend):
    sc.case_kde_measurement_and_anyn(oracle_backend)


def test_independence(oracle_backend):
    sc.case_independence(oracle_backend)


# ---- the power checks: no backend ------------------------------------------------------------------------------------------------
# Each one draws, with numpy, a sample of the size the backend case pools -- once from the right law (the battery must pass:
# the thresholds are quantiles, a right sample exceeds one with probability ALPHA) and once from a slightly wrong one (the
# named statistic must reject).  A case that could not reject its perturbation would get more draws, never a wider threshold.
POOL = sc.NP * sc.OPS


def rejects(match, fn, *args, **kw):
    """the battery must reject, and the statistic named by `match` must be among those that do (None: any)"""
    sc.collected = []
    try:
        with pytest.raises(AssertionError, match=match):
            fn(*args, **kw)
            assert not sc.collected, "\n".join(sc.collected)
    finally:
        sc.collected = None


@pytest.mark.parametrize("manifold", MANIFOLDS)
def test_power_gaussian_sigma_off_by_one_percent(manifold):
    rng = np.random.default_rng(100 + manifold)
    mu, L, circ = sc.GAUSS[manifold]
    n = rng.normal(size=(POOL, len(mu)))
    sc.gaussian_ok(mu + n @ np.asarray(L).T, mu, L, "right law", ())
    Lw = np.array(L, dtype=float)
    Lw[-1, -1] *= 1.01  # the last coordinate's own sigma
    rejects(r"moment\[", sc.gaussian_ok, mu + n @ Lw.T, mu, L, "sigma + 1 %", ())
    Lw[-1, -1] = L[-1][-1] * 0.99
    rejects(r"moment\[", sc.gaussian_ok, mu + n @ Lw.T, mu, L, "sigma - 1 %", ())


@pytest.mark.parametrize("manifold", [abi.EUCLID2, abi.EUCLID3, abi.SE2])
def test_power_cholesky_entry_dropped_or_transposed(manifold):
    rng = np.random.default_rng(110 + manifold)
    mu, L, _ = sc.GAUSS[manifold]
    n = rng.normal(size=(POOL, len(mu)))
    D = len(mu)
    for i in range(D):
        for j in range(i):
            Lw = np.array(L, dtype=float)
            Lw[i, j] = 0.0
            rejects(r"cov\[|whitened", sc.gaussian_ok, mu + n @ Lw.T, mu, L, f"L[{i},{j}] dropped", ())
    rejects(r"cov\[|whitened", sc.gaussian_ok, mu + n @ np.asarray(L), mu, L, "factor read transposed", ())


def test_power_uniform_and_rayleigh_scale_off_by_one_percent():
    rng = np.random.default_rng(120)
    u = rng.uniform(size=POOL)
    sc.uniform_ok(2.0 + 3.0 * u, 2.0, 5.0, "right law")
    rejects("KS", sc.uniform_ok, 2.0 + 3.0 * 0.99 * u, 2.0, 5.0, "width - 1 %")
    rejects(None, sc.uniform_ok, 2.0 + 3.0 * 1.01 * u, 2.0, 5.0, "width + 1 %")  # (leaves the support)
    r = np.sqrt(-2.0 * np.log(u))
    sc.rayleigh_ok(1.7 * r, 1.7, "right law")
    rejects("second moment", sc.rayleigh_ok, 1.7 * 1.01 * r, 1.7, "sigma + 1 %")
    rejects("second moment", sc.rayleigh_ok, 1.7 * 0.99 * r, 1.7, "sigma - 1 %")


def test_power_pmf_entry_off_by_one_hundredth():
    rng = np.random.default_rng(130)
    # the tabulated samplers (204 800 draws each)
    for name, w in sc.table_pmfs(sc.NP).items():
        n = 400 * sc.NP
        sc.chi2_ok(rng.multinomial(n, w), w, f"right law, table {name}")
        pos = np.flatnonzero(w)
        ww = w * (1.0 - w[pos[0]] - 0.01) / (1.0 - w[pos[0]])  # one entry + 0.01, taken off the others in proportion
        ww[pos[0]] = w[pos[0]] + 0.01
        rejects("chi2", sc.chi2_ok, rng.multinomial(n, ww), w, f"table {name}, an entry + 0.01")
        ww = w.copy()
        ww[pos[-1]] = 0.0  # the last positive entry never drawn
        rejects("chi2", sc.chi2_ok, rng.multinomial(n, ww / ww.sum()), w, f"table {name}, last entry never drawn")
    # mixture labels (819 200 draws) and the hypothesis draws (307 200)
    for n, pmfs in ((POOL, [sc.mixture_pmf(w) for w in sc.MIXTURES.values()]),
                    (600 * sc.NP, [np.array([nh, 1 - nh]) for nh in (0.1, 0.5, 0.9)]
                     + [sc.hypothesis_pmf(mh, sf) for mh in ([0.0, 0.3, 0.7], [0.0, 0.2, 0.3, 0.5]) for sf in (0, 1)])):
        for p in pmfs:
            sc.chi2_ok(rng.multinomial(n, p), p, "right law")
            pos = np.flatnonzero(p)
            pw = p.copy()
            pw[pos[0]] -= 0.01
            pw[pos[-1]] += 0.01
            rejects("chi2", sc.chi2_ok, rng.multinomial(n, pw), p, "an entry off by 0.01")
    # a zero-weight entry drawn once
    rejects("zero-probability", sc.chi2_ok, [500, 1, 499], [0.5, 0.0, 0.5], "a zero weight drawn")


def test_power_last_kernel_never_picked():
    rng = np.random.default_rng(140)
    n = sc.BELIEF_OPS * sc.NP
    for cd in (2, 100, sc.NP - 1, sc.NP):
        sc.kernel_pick_ok(rng.integers(0, cd, n), cd, "right law")
        rejects(None, sc.kernel_pick_ok, rng.integers(0, cd - 1, n), cd, "last kernel never picked")
        rejects(None, sc.kernel_pick_ok, rng.integers(1, cd, n), cd, "first kernel never picked")
        rejects("beyond", sc.kernel_pick_ok, rng.integers(0, cd + 1, n), cd, "one past the end")
    # the chi-square alone (without the reachability assert) sees it too
    cnt = np.bincount(rng.integers(0, sc.NP - 1, n), minlength=sc.NP)
    rejects("chi2", sc.chi2_ok, cnt, np.full(sc.NP, 1.0 / sc.NP), "last of 512 kernels never picked")


def test_power_kernel_noise_sigma_off_by_one_percent():
    rng = np.random.default_rng(150)
    n = sc.BELIEF_OPS * (sc.NP - 1 + sc.NP - 2 + sc.NP - 100 + 1)  # the smallest pooled noise sample: the top-up cases
    w = rng.normal(size=(n, 3))
    sc.kernel_noise_ok(w, "right law")
    rejects("variance", sc.kernel_noise_ok, w * [1.0, 1.0, 1.01], "bandwidth + 1 %")
    rejects("variance", sc.kernel_noise_ok, w * [0.99, 1.0, 1.0], "bandwidth - 1 %")
    w2 = w.copy()
    w2[:, 2] = np.sqrt(1 - 1e-4) * w[:, 2] + 0.01 * w[:, 0]
    rejects("correlation", sc.kernel_noise_ok, w2, "coordinates correlated at 0.01")


def test_power_entropy_width_off_by_two_percent():
    rng = np.random.default_rng(160)
    n = POOL // 2  # nullhypo = 0.5
    e = rng.uniform(-0.5, 0.5, (n, 3))
    sc.unit_entropy_ok(e, "right law")
    rejects("coordinate", sc.unit_entropy_ok, e * [1.0, 0.98, 1.0], "entropy 2 % narrow")
    rejects("of the width", sc.unit_entropy_ok, e * [1.0, 1.0, 1.02], "entropy 2 % wide")
    # null particles spread over the wrong width because the spread statistic is wrong: the same thing
    rejects(None, sc.unit_entropy_ok, e * np.sqrt(511.0 / 512.0) ** 20, "spread off by 2 %")


def test_power_lag_one_correlation_of_one_hundredth():
    rng = np.random.default_rng(170)
    from scipy import stats
    a, b = rng.normal(size=POOL), rng.normal(size=POOL)
    sc.independent_uniforms_ok(stats.norm.cdf(a), stats.norm.cdf(b), "right law")
    rejects("correlation", sc.independent_uniforms_ok, stats.norm.cdf(a), stats.norm.cdf(0.01 * a + np.sqrt(1 - 1e-4) * b), "correlation 0.01")
    # overlapping counters: one draw in a hundred is the neighbour's
    u, v = rng.uniform(size=POOL), rng.uniform(size=POOL)
    v2 = np.where(rng.uniform(size=POOL) < 0.01, u, v)
    rejects(None, sc.independent_uniforms_ok, u, v2, "1 % of the draws shared")


def test_power_label_leaks_into_the_value():
    rng = np.random.default_rng(180)
    for w in ([0.35, 0.65], [0.1, 0.2, 0.3, 0.4]):
        w = np.asarray(w)
        ul, uv = rng.uniform(size=POOL), rng.uniform(size=POOL)
        lab = np.searchsorted(np.cumsum(w), ul, side="right")
        from scipy import stats
        sc.labels_ok(100.0 * lab + stats.norm.ppf(uv), w, "right law")
        leak = np.where(rng.uniform(size=POOL) < 0.01, ul, uv)  # 1 % of the values reuse the label's uniform
        rejects("label x quantile", sc.labels_ok, 100.0 * lab + stats.norm.ppf(leak), w, "label leaks into 1 % of the values")


def test_power_stream_tolerances():
    """stream_particle_ok, the assert of case_stream_is_philox, on values made here with libm from the Python stream: it takes
    the right ones, and refuses a uniform one cell of 2^-53 off, a Rayleigh draw 4 ulps off, a Gaussian coordinate 1e-13 off
    (relatively; its tolerance is a few tens of ulps: the sincos bound is absolute, ~2 pi eps r), a draw that read the factor
    transposed, the next particle's draw and the next seed's"""
    import math

    def draws(s, n, transpose=False):
        ua, ub = sc.uniform_pair(s, n, sc.PURP_MEAS, 0)
        uc, ud = sc.uniform_pair(s, n, sc.PURP_MEAS, 1)
        nn = [math.sqrt(-2 * math.log(u1)) * f(2 * math.pi * u2) for u1, u2 in ((ua, ub), (uc, ud)) for f in (math.cos, math.sin)]
        g = []
        for mu, L in sc._G.values():
            L = np.asarray(L).T if transpose else np.asarray(L)
            g.append(np.asarray(mu) + L @ np.asarray(nn[:len(mu)]))
        return ua, sc._RAY_SIGMA * math.sqrt(-2 * math.log(ua)), g

    for s in sc.STREAM_SEEDS:
        for n in (0, 1, 63, 64, 511):
            uni, ray, g = draws(s, n)
            sc.stream_particle_ok(s, n, uni, ray, g)
            with pytest.raises(AssertionError, match="uniform"):
                sc.stream_particle_ok(s, n, uni + 2.0 ** -53, ray, g)
            with pytest.raises(AssertionError, match="rayleigh"):
                sc.stream_particle_ok(s, n, uni, ray * (1 + 4 * 2.0 ** -52), g)
            for gi in range(3):
                for i in range(gi + 1):
                    bad = [x.copy() for x in g]
                    bad[gi][i] += 1e-13 * max(1.0, abs(bad[gi][i]))
                    with pytest.raises(AssertionError, match="gaussian"):
                        sc.stream_particle_ok(s, n, uni, ray, bad)
            with pytest.raises(AssertionError, match="gaussian"):
                sc.stream_particle_ok(s, n, uni, ray, draws(s, n, transpose=True)[2])
            with pytest.raises(AssertionError):
                sc.stream_particle_ok(s, n, *draws(s, n + 1))
            with pytest.raises(AssertionError):
                sc.stream_particle_ok(s, n, *draws((s + 1) & (2 ** 64 - 1), n))


def test_spread_restatement_against_closed_forms():
    """std_basic_spread of sampling_cases.py on points whose answer is known by hand"""
    assert abs(sc.std_basic_spread(abi.EUCLID1, np.array([[1.0], [3.0]])) - np.sqrt(2.0)) < 1e-15
    assert abs(sc.std_basic_spread(abi.EUCLID2, np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0], [2.0, 2.0]])) - np.sqrt(8.0 / 3.0)) < 1e-15
    assert abs(sc.std_basic_spread(abi.CIRCULAR, np.array([[3.1], [-3.1]])) - np.sqrt(2.0) * (np.pi - 3.1)) < 1e-13  # across the seam
    assert abs(sc.std_basic_spread(abi.SE2, np.array([[0.0, 0.0, 0.1], [0.0, 0.0, -0.1]])) - np.sqrt(2 * 2 * 0.01)) < 1e-15
    assert sc.std_basic_spread(abi.EUCLID3, np.zeros((5, 3))) == 1.0


def test_false_alarm_budget():
    """ALPHA = 1e-4 / BUDGET per statistical assert; sc._spend itself refuses the assert that would exceed the budget, in any
    order of the tests -- here only that the level is what the header says"""
    assert sc.ALPHA * sc.BUDGET == sc.ALPHA_FILE == 1e-4 and sc.spent[0] <= sc.BUDGET
