"""Mixture summaries on the host: the numpy restatement of the definition (incrementalinference.jl_amd/mixture.py) against closed
forms -- one component is the mean and the covariance, separated clusters keep their shares exactly, a cloud across +-pi is one
component, J never decreases on Euclidean manifolds --, the table of tests/modes_cases.py, the way back into a graph (`asPrior`),
and the degenerate inputs."""
import numpy as np
import pytest

import mixture_cases as xc
import modes_cases as mc
import ppe_cases as pc
from parity_utils import abi, iif

mixture = iif.mixture
EUCLID = (abi.EUCLID1, abi.EUCLID2, abi.EUCLID3)


def _one_component(c):
    mu = np.zeros((abi.MIX_MAX, abi.MAXD))
    return np.zeros(c, dtype=np.int32), mu


@pytest.mark.parametrize("manifold", EUCLID)
def test_one_component_is_the_mean_and_the_covariance(manifold):
    rng = np.random.default_rng(10 + manifold)
    D, c = abi.MANIFOLD_DIM[manifold], 200
    X = pc.cloud("gaussian", manifold, c, rng) @ (np.eye(D) + 0.3 * np.triu(np.ones((D, D)), 1))  # correlated coordinates
    bw = pc.hand_bandwidth(manifold)
    fit = mixture.mixture_numpy(manifold, X, bw, *_one_component(c))
    mean, cov = iif.beliefstats.meancov_numpy(manifold, X)
    want = (c - 1) / c * cov + np.diag(bw * bw)
    assert fit.n_comp == 1 and fit.weight[0] == 1.0 and fit.count[0] == c and fit.converged == 1 and fit.iters == 2
    assert np.all(np.abs(fit.mean[0, :D] - mean) <= 1e-12 * np.abs(mean)), (fit.mean[0], mean)
    assert np.all(np.abs(fit.cov[0, :D, :D] - want) <= 1e-12 * np.abs(want).max()), (fit.cov[0], want)
    assert np.all(fit.mean[1:] == 0) and np.all(fit.cov[1:] == 0) and np.all(fit.cov[0, D:] == 0) and np.all(fit.labels == 0)


@pytest.mark.parametrize("manifold", EUCLID)
def test_separated_clusters_keep_their_shares_exactly(manifold):
    rng = np.random.default_rng(20 + manifold)
    D = abi.MANIFOLD_DIM[manifold]
    X = rng.normal(0.0, 0.3, (200, D))
    X[70:, 0] += 100.0
    lab = np.where(np.arange(200) < 70, 1, 0).astype(np.int32)  # (the starting index is not the rank)
    mu = np.zeros((abi.MIX_MAX, abi.MAXD))
    mu[0, 0] = 100.0
    fit = mixture.mixture_numpy(manifold, X, pc.hand_bandwidth(manifold), lab, mu)
    assert fit.n_comp == 2 and fit.weight[0] == 0.65 and fit.weight[1] == 0.35 and fit.count.tolist()[:2] == [130, 70]
    for q, rows in enumerate((slice(70, 200), slice(0, 70))):
        want = X[rows].mean(axis=0)
        assert np.all(np.abs(fit.mean[q, :D] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (q, fit.mean[q], want)
    # the responsibilities underflow to exact zeros
    assert set(np.unique(fit.resp[:, :2]).tolist()) == {0.0, 1.0} and np.array_equal(fit.labels, np.where(np.arange(200) < 70, 1, 0))
    assert fit.rank.tolist()[:2] == [0, 1] and fit.iters == 2 and fit.converged == 1


@pytest.mark.parametrize("manifold", (abi.CIRCULAR, abi.SE2))
def test_a_cloud_across_pi_is_one_component(manifold):
    rng = np.random.default_rng(30 + manifold)
    D, c, sigma = abi.MANIFOLD_DIM[manifold], 200, 0.3
    k = pc.circular_coords(manifold)[0]
    X = rng.normal(0.3, 0.5, (c, D))
    X[:, k] = pc.wrap(rng.normal(np.pi, sigma, c))
    assert (X[:, k] > 0).sum() > 50 and (X[:, k] < 0).sum() > 50  # the cloud does straddle the cut
    bw = pc.hand_bandwidth(manifold)
    lab, mu = _one_component(c)
    mu[0, k] = 3.0
    fit = mixture.mixture_numpy(manifold, X, bw, lab, mu)
    assert fit.n_comp == 1 and fit.iters == 2 and fit.converged == 1
    assert abs(pc.wrap(fit.mean[0, k] - np.pi)) <= 4 * sigma / np.sqrt(c), fit.mean[0]
    dl = pc.wrap(X[:, k] - fit.mean[0, k])
    assert abs(fit.cov[0, k, k] - (np.mean(dl * dl) + bw[k] ** 2)) <= 1e-12, (fit.cov[0, k, k], np.mean(dl * dl) + bw[k] ** 2)
    assert abs(np.mean(dl)) <= 1e-12  # the mean is the circular mean: the deviations about it cancel


def _euclid_cases():
    for m in EUCLID:
        rng = np.random.default_rng(40 + m)
        for K in (2, 3, 8):
            yield f"blobs manifold {m} K={K}", (m, *xc.blobs(m, 200, K, rng))
        yield f"starved manifold {m}", (m, *xc.starved(m, 150, rng))
        for kind in mc.TABLE_CLOUDS:
            X, bw, scale, _ = mc.make(kind, m, 200, rng)
            bm = iif.modes.modes_numpy(m, X, bw, scale)
            yield f"{kind} manifold {m}", (m, X, bw, *mixture.starting_from_modes(bm, abi.MIX_MAX))


def test_the_objective_never_decreases_on_euclidean_manifolds():
    worst = 0.0
    for what, (m, X, bw, lab, mu) in _euclid_cases():
        fit = mixture.mixture_numpy(m, X, bw, lab, mu, tol=1e-10)
        J = np.asarray(fit.history)
        assert len(J) == fit.iters >= 2 and np.all(np.isfinite(J)), what
        steps = np.diff(J)
        worst = min(worst, float(steps.min()))
        assert np.all(steps >= -1e-12 * np.maximum(1.0, np.abs(J[1:]))), (what, steps.min())
    print(f"the worst step of J over every Euclidean case: {worst:.3e}")


@pytest.mark.parametrize("manifold", xc.MANIFOLDS)
def test_every_table_cloud_has_the_components_the_table_requires(manifold):
    rng = np.random.default_rng(50 + manifold)
    for kind in mc.TABLE_CLOUDS + (("doors4",) if manifold == abi.CIRCULAR else ()):
        X, bw, scale, heavy = mc.make(kind, manifold, 200, rng)
        bm = mixture.belief_mixture(manifold, pc.to_points(manifold, X), bw, bwScale=scale)
        assert bm.n_comp == mc.required_modes(kind, manifold) == bm.modes.n_modes, (kind, bm.n_comp)
        assert bm.converged and bm.n_dropped == 0 and abs(bm.weights.sum() - 1) <= 1e-14 and np.all(np.diff(bm.weights) <= 0)
        assert bm.means.shape == (bm.n_comp, abi.MANIFOLD_DIM[manifold]) and int(bm.counts.sum()) == 200
        assert np.array_equal(np.bincount(bm.labels, minlength=bm.n_comp), bm.counts)
        if kind == "two_cluster":
            one = mixture.belief_mixture(manifold, pc.to_points(manifold, X), bw, maxComponents=1, bwScale=scale)
            assert one.n_comp == 1 and bm.objective > one.objective, (bm.objective, one.objective)
            assert np.array_equal(bm.labels, np.where(heavy, 0, 1))


def test_a_run_is_the_prefix_of_a_longer_one():
    rng = np.random.default_rng(60)
    X, bw, lab, mu = xc.blobs(abi.EUCLID2, 150, 3, rng)
    at = mixture.mixture_numpy(abi.EUCLID2, X, bw, lab, mu, tol=0.0, at=(1, 2, 7))
    for t in (1, 2, 7):
        one = mixture.mixture_numpy(abi.EUCLID2, X, bw, lab, mu, tol=0.0, max_iter=t)
        assert one.iters == t == at[t].iters and one.converged == 0
        for f in ("weight", "mean", "cov", "count", "labels", "resp"):
            assert np.array_equal(getattr(one, f), getattr(at[t], f)), (t, f)
        assert one.objective == at[t].objective


@pytest.mark.parametrize("manifold", xc.MANIFOLDS)
def test_as_prior_gives_the_components_back(manifold):
    rng = np.random.default_rng(70 + manifold)
    vt = {abi.EUCLID1: iif.ContinuousScalar, abi.EUCLID2: iif.ContinuousEuclid(2), abi.EUCLID3: iif.ContinuousEuclid(3),
          abi.CIRCULAR: iif.Circular, abi.SE2: iif.SpecialEuclidean2}[manifold]
    D = abi.MANIFOLD_DIM[manifold]
    X, bw, lab, mu = xc.blobs(manifold, 200, 3, rng)
    fit = mixture.mixture_numpy(manifold, X, bw, lab, mu)
    bm = mixture.mixture_from_record(manifold, fit, fit.labels, 200)
    prior = bm.asPrior(vt)
    comps = prior.components()
    assert prior.is_prior and len(comps) == 3 == bm.n_comp
    for (w, m, L, fam), wk, mk, Sk in zip(comps, bm.weights, bm.means, bm.covs):
        assert abs(w - wk) <= 1e-15 and np.array_equal(np.asarray(m).reshape(-1), mk) and fam == abi.DIST_GAUSSIAN
        L = np.asarray(L).reshape(D, D)
        assert np.abs(L @ L.T - Sk).max() <= 1e-12 and np.all(np.triu(L, 1) == 0)
    for (w, m, L), wk in zip(bm.components(), bm.weights):
        assert w == wk and L.shape == (D, D)
    with pytest.raises(ValueError, match="manifold"):
        bm.asPrior(iif.ContinuousEuclid(2) if manifold != abi.EUCLID2 else iif.ContinuousScalar)
    # the density the prior stands for: greatest at the heaviest mean among the means, finite everywhere
    ld = bm.logdensity(pc.to_points(manifold, np.vstack([bm.means, X[:5]])))
    assert ld.shape == (8,) and np.all(np.isfinite(ld))


def test_five_components_do_not_fit_a_prior():
    rng = np.random.default_rng(80)
    X, bw, lab, mu = xc.blobs(abi.EUCLID2, 200, 5, rng)
    fit = mixture.mixture_numpy(abi.EUCLID2, X, bw, lab, mu)
    bm = mixture.mixture_from_record(abi.EUCLID2, fit, fit.labels, 200)
    assert bm.n_comp == 5
    with pytest.raises(ValueError, match="maxComponents"):
        bm.asPrior(iif.ContinuousEuclid(2))


def test_degenerate_inputs():
    rng = np.random.default_rng(90)
    for m in xc.MANIFOLDS:
        D = abi.MANIFOLD_DIM[m]
        X, bw, lab, mu = xc.blobs(m, 100, 2, rng)
        for bad in (0.0, np.nan, np.inf, -1.0):
            h = bw.copy()
            h[-1] = bad
            fit = mixture.mixture_numpy(m, X, h, lab, mu)
            assert fit.n_comp == 0 and fit.iters == 0 and np.all(fit.labels == -1) and len(fit.labels) == 100 and np.all(fit.count == 0)
            assert np.all(np.isnan(fit.weight)) and np.all(np.isnan(fit.mean)) and np.all(np.isnan(fit.cov)) and np.isnan(fit.objective)
            bm = mixture.belief_mixture(m, pc.to_points(m, X), h)
            assert bm.n_comp == 0 and np.all(bm.labels == -1) and np.isnan(bm.objective)
        none = mixture.mixture_numpy(m, X, bw, np.full(100, -1), mu)
        assert none.n_comp == 0 and np.all(np.isnan(none.weight)) and np.all(none.labels == -1)
        # one point: one component, the point itself, Sigma = H
        one = mixture.mixture_numpy(m, X[:1], bw, [0], X[:1])
        assert one.n_comp == 1 and one.weight[0] == 1.0 and np.array_equal(one.mean[0, :D], X[0]) and one.count[0] == 1
        assert np.array_equal(one.cov[0, :D, :D], np.diag(bw * bw)) and one.iters == 2 and one.converged == 1
        # a component starved below half a particle is dropped and counted
        Xs, bws, labs, mus = xc.starved(m, 150, rng)
        st = mixture.mixture_numpy(m, Xs, bws, labs, mus)
        assert st.n_comp == 2 and st.n_dropped == 1 and st.n_drop_max < 0.25 and st.n_live_min >= 1.0 and st.rank[2] == -1
        assert np.all(st.weight[2:] == 0) and abs(st.weight[:2].sum() - 1) <= 1e-15 and np.all((st.labels >= 0) & (st.labels < 2))


def test_the_options_are_checked():
    rng = np.random.default_rng(100)
    X, bw, lab, mu = xc.blobs(abi.EUCLID1, 50, 2, rng)
    for kw in (dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf), dict(max_iter=0), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            mixture.mixture_numpy(abi.EUCLID1, X, bw, lab, mu, **kw)
    for kw in (dict(maxComponents=0), dict(maxComponents=9), dict(tol=-1.0), dict(maxIter=0), dict(bwScale=0.0)):
        with pytest.raises(ValueError):
            mixture.belief_mixture(abi.EUCLID1, X, bw, **kw)
    with pytest.raises(ValueError, match="label"):
        mixture.mixture_numpy(abi.EUCLID1, X, bw, np.full(50, 8), mu)
    full = mixture.mixture_numpy(abi.EUCLID1, X, bw, lab, mu, tol=0.0, max_iter=5)
    assert full.iters == 5 and full.converged == 0  # tol = 0: max_iter iterations


def test_the_mirror_without_a_backend():
    fg = iif.initfg(iif.SolverParams(N=100))
    rng = np.random.default_rng(110)
    for i, m in enumerate((iif.ContinuousEuclid(2), iif.Circular)):
        iif.addVariable(fg, f"x{i}", m)
        X, bw, _, heavy = mc.make("two_cluster", m.manifold, 100, rng)
        iif.setValKDE(fg, f"x{i}", pc.to_points(m.manifold, X), bw)
    both = iif.fitBeliefMixtureAll(fg, bwScale=1.0)
    assert list(both) == ["x0", "x1"]
    for v in ("x0", "x1"):
        one = iif.fitBeliefMixture(fg, v, bwScale=1.0)
        bel = iif.getBelief(fg, v).mixture(bwScale=1.0)
        assert both[v].n_comp == 2 and both[v].weights.tobytes() == one.weights.tobytes() == bel.weights.tobytes()
        assert both[v].means.tobytes() == one.means.tobytes() and both[v].covs.tobytes() == bel.covs.tobytes()
        assert iif.fitBeliefMixture(fg, v, maxComponents=1, bwScale=1.0).n_comp == 1
