"""-m gpu: Gaussian-mixture summaries of beliefs on the device (nbp_run_mixture / nbp_kde_mixture, csrc/nbp_mixture.h) through the
C ABI and through the mirror, held to the numpy restatement on the slot as read back by the criteria of tests/mixture_cases.py:
weights, means, covariances and J within 16 max(|float64 - long double restatement|, 4 ulp); n_comp, n_dropped, iteration counts,
labels and counts equal (labels and counts but for close calls of the restatement).  Every bandwidth is set by hand.  The runs are
at tol = 0 with max_iter in 1, 2, 10, 50, so that a stopping decision cannot hide in the comparison; one converged run per manifold
follows."""
import ctypes as C

import numpy as np
import pytest

import mixture_cases as xc
import ppe_cases as pc
from parity_utils import abi, coords, iif

pytestmark = pytest.mark.gpu
mixture = iif.mixture


def _load(be, items, seed):
    """items = [(manifold, K, count)] -> slot i holds belief i (blobs; K = 0: starved; two points in two components: far_pair);
    returns (slots, manifolds, label rows n x N, means n x 8 x 3)"""
    rng = np.random.default_rng(seed)
    made = [xc.far_pair(m) if (c == 2 and K == 2) else (xc.starved(m, c, rng) if K == 0 else xc.blobs(m, c, K, rng)) for m, K, c in items]
    slots, mans = list(range(len(items))), [m for m, _, _ in items]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), bw, None) for m, (X, bw, _, _) in zip(mans, made)])
    lab = np.full((len(items), be.N), -1, dtype=np.int32)
    mu = np.zeros((len(items), abi.MIX_MAX, abi.MAXD))
    for i, (X, _, li, mi) in enumerate(made):
        lab[i, :len(li)], mu[i] = li, mi
    return slots, mans, lab, mu


def _check_prefixes(be, items, slots, mans, lab, mu, iters=xc.ITERS):
    """tol = 0 runs of max_iter = every entry of `iters`, each against the restatement's state after as many iterations"""
    back = be.beliefs_read(slots, mans)
    refs = []
    for i, (m, K, c) in enumerate(items):
        pts, bw, _ = back[i]
        assert len(pts) == c and np.all(lab[i, c:] == -1)  # rows beyond the count hold -1
        refs.append(xc.restate(m, coords(m, pts), bw, lab[i, :c], mu[i], tol=0.0, at=iters))
    assert max(c for _, _, c in items) < 60 or any(np.any(lab[i, :c] == -1) for i, (_, _, c) in enumerate(items))  # -1 inside a row too
    worst = 0.0
    for t in iters:
        recs, out = be.run_mixture(slots, mans, lab, mu, tol=0.0, max_iter=t)
        for i, (m, K, c) in enumerate(items):
            f64, f80 = refs[i][0][t], refs[i][1][t]
            assert f64.iters == t and f64.converged == 0
            worst = max(worst, xc.check_device(m, recs[i], out[i], f64, f80, what=f"[{i}] manifold {m} K={K} c={c} N={be.N} max_iter={t}"))
    print(f"N={be.N}: {len(items)} beliefs x {len(iters)} runs, the greatest error is {worst:.3f} of its bound")


@pytest.mark.parametrize("N", xc.SIZES)
def test_every_manifold_and_component_count_at_full_count(hip_backend, N):
    items = [(m, K, N) for m in xc.MANIFOLDS for K in (1, 2, 8)]
    be = hip_backend(N, len(items))
    try:
        _check_prefixes(be, items, *_load(be, items, 1000 + N))
    finally:
        be.close()


def test_counts_below_the_context_size(hip_backend):
    items = [(m, 1, 1) for m in xc.MANIFOLDS] + [(m, K, 2) for m in xc.MANIFOLDS for K in (1, 2)]
    items += [(m, K, c) for m in xc.MANIFOLDS for c in (63, 150) for K in (1, 2, 8)] + [(m, 0, 150) for m in xc.MANIFOLDS]
    be = hip_backend(200, len(items))
    try:
        slots, mans, lab, mu = _load(be, items, 11)
        _check_prefixes(be, items, slots, mans, lab, mu)
        recs, _ = be.run_mixture(slots, mans, lab, mu)
        assert all(recs[i]["n_dropped"] == 1 and recs[i]["n_comp"] == 2 for i, (_, K, _) in enumerate(items) if K == 0)
        back = be.beliefs_read(slots, mans)
        for i, (m, K, c) in enumerate(items):
            if c == 1:  # one component: the point itself, Sigma = H
                D, X = abi.MANIFOLD_DIM[m], coords(m, back[i][0])
                bw = back[i][1]
                assert recs[i]["n_comp"] == 1 and recs[i]["weight"][0] == 1.0 and recs[i]["count"][0] == 1
                assert np.abs(xc.coord_diff(m, recs[i]["mean"][0, :D], X[0])).max() <= 1e-15
                assert np.array_equal(recs[i]["cov"][0, :D, :D], np.diag(bw * bw)), (recs[i]["cov"][0], bw)
    finally:
        be.close()


@pytest.mark.parametrize("manifold", xc.MANIFOLDS)
def test_a_converged_run(hip_backend, manifold):
    """the default stopping rule: the device stops within one iteration of the restatement, and what it delivers is the
    restatement's state after as many iterations as the device ran"""
    items = [(manifold, 3, 200)]
    be = hip_backend(200, 1)
    try:
        slots, mans, lab, mu = _load(be, items, 31 + manifold)
        pts, bw, _ = be.beliefs_read(slots, mans)[0]
        X = coords(manifold, pts)
        ref = mixture.mixture_numpy(manifold, X, bw, lab[0], mu[0])
        recs, out = be.run_mixture(slots, mans, lab, mu)
        it = int(recs[0]["iters"])
        print(f"manifold {manifold}: the restatement stops after {ref.iters} iterations, the device after {it}")
        assert ref.converged == 1 and 2 < ref.iters < abi.MIX_MAX_ITER and recs[0]["converged"] == 1
        assert abs(it - ref.iters) <= 1
        f64, f80 = xc.restate(manifold, X, bw, lab[0], mu[0], tol=0.0, at=(it,))
        f64[it].converged = f80[it].converged = 1
        f64[it].iters = ref.iters  # (within +-1: asserted above and again by check_device)
        xc.check_device(manifold, recs[0], out[0], f64[it], f80[it], what=f"manifold {manifold} converged", converged_run=True)
    finally:
        be.close()


def test_a_mixed_batch_equals_the_single_launches(hip_backend):
    rng = np.random.default_rng(5)
    items = [(int(rng.choice(xc.MANIFOLDS)), int(rng.choice((1, 2, 3, 5, 8))), int(rng.choice((200, 200, 150, 63, 7)))) for _ in range(40)]
    be = hip_backend(200, len(items))
    try:
        slots, mans, lab, mu = _load(be, items, 6)
        recs, out = be.run_mixture(slots, mans, lab, mu, max_iter=60)
        assert len({int(r["iters"]) for r in recs}) > 3  # the beliefs of one launch stop on their own
        for i in range(len(items)):
            one, lone = be.run_mixture([slots[i]], [mans[i]], lab, mu[i:i + 1], max_iter=60, rows=[i])
            assert one[0].tobytes() == recs[i].tobytes() and np.array_equal(lone[0], out[i]), (i, items[i])
        # any order, any row table
        perm = rng.permutation(len(items))
        again, lagain = be.run_mixture([slots[i] for i in perm], [mans[i] for i in perm], lab, mu[perm], max_iter=60, rows=perm)
        assert again.tobytes() == recs[perm].tobytes() and np.array_equal(lagain, out[perm])
    finally:
        be.close()


@pytest.mark.parametrize("manifold", xc.MANIFOLDS)
def test_the_host_buffer_form_equals_the_slot_form(hip_backend, manifold):
    be = hip_backend(200, 2)
    try:
        rng = np.random.default_rng(70 + manifold)
        for c in (200, 77):
            X, bw, lab, mu = xc.blobs(manifold, c, 3, rng)
            pts = pc.to_points(manifold, X)
            rec, out = be.kde_mixture(manifold, pts, bw, lab, mu)
            be.belief_write(1, manifold, pts, bw)
            row = np.full((1, be.N), -1, dtype=np.int32)
            row[0, :c] = lab
            recs, outs = be.run_mixture([1], [manifold], row, mu[None])
            assert rec.tobytes() == recs[0].tobytes() and np.array_equal(out, outs[0, :c]) and len(out) == c
            assert rec["n_comp"] == 3 and rec["iters"] >= 2
    finally:
        be.close()


def test_degenerate_beliefs(hip_backend):
    be = hip_backend(64, 3)
    try:
        rng = np.random.default_rng(3)
        X, bw, lab, mu = xc.blobs(abi.EUCLID2, 64, 2, rng)
        be.beliefs_write([0, 1, 2], [abi.EUCLID2] * 3, [(X, np.array([0.1, np.inf]), None), (X, np.array([0.0, 0.1]), None), (X, bw, None)])
        rows = np.stack([lab, lab, np.full(64, -1, dtype=np.int32)])
        recs, out = be.run_mixture([0, 1, 2], [abi.EUCLID2] * 3, rows, np.stack([mu] * 3))
        for r in recs:
            assert r["n_comp"] == 0 and r["iters"] == 0 and r["converged"] == 0 and r["n_dropped"] == 0 and np.all(r["count"] == 0)
            assert np.all(np.isnan(r["weight"])) and np.all(np.isnan(r["mean"])) and np.all(np.isnan(r["cov"])) and np.isnan(r["objective"])
        assert np.all(out == -1)
    finally:
        be.close()


def _raw(be, slots, mans, lab, rows, mu, opts, recs=True, n=None):
    """nbp_run_mixture called directly -> its status"""
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    s, m, r = (np.ascontiguousarray(a, dtype=np.int32) for a in (slots, mans, rows))
    lab, mu = np.ascontiguousarray(lab, dtype=np.int32), np.ascontiguousarray(mu, dtype=np.float64)
    out = np.zeros(max(len(s), 1), dtype=be.MIX_REC)
    return be.lib.nbp_run_mixture(be._ctx, s.ctypes.data_as(ip), m.ctypes.data_as(ip), len(s) if n is None else n, lab.ctypes.data_as(ip),
                                  r.ctypes.data_as(ip), mu.ctypes.data_as(dp), C.byref(opts) if opts is not None else None,
                                  out.ctypes.data_as(C.POINTER(abi.MixtureRec)) if recs else None, None), out


def test_refusals(hip_backend):
    """every refused argument returns its status before anything is launched: the records handed in stay untouched, and the
    context serves the next call"""
    ERR_ARG, ERR_RANGE = -1, -4
    be = hip_backend(64, 2)
    try:
        rng = np.random.default_rng(9)
        X, bw, lab, mu = xc.blobs(abi.EUCLID2, 64, 2, rng)
        be.belief_write(0, abi.EUCLID2, X, bw)
        good = abi.MixtureOpts(tol=1e-8, max_iter=20)
        rows2 = np.stack([lab, lab])
        assert _raw(be, [0], [abi.EUCLID2], rows2, [0], mu[None], good)[0] == 0
        assert _raw(be, [0], [abi.EUCLID2], rows2, [0], mu[None], None)[0] == 0  # the defaults
        bad_opts = [abi.MixtureOpts(tol=-1e-9, max_iter=20), abi.MixtureOpts(tol=float("nan"), max_iter=20),
                    abi.MixtureOpts(tol=float("inf"), max_iter=20), abi.MixtureOpts(tol=1e-8, max_iter=0),
                    abi.MixtureOpts(tol=1e-8, max_iter=-3)]
        for o in bad_opts:
            rc, out = _raw(be, [0], [abi.EUCLID2], rows2, [0], mu[None], o)
            assert rc == ERR_ARG and not out.tobytes().strip(b"\0") and b"mixture" in be.lib.nbp_last_error(), (o.tol, o.max_iter)
        for v in (abi.MIX_MAX, -2):
            bad = rows2.copy()
            bad[1, 63] = v
            assert _raw(be, [0], [abi.EUCLID2], bad, [1], mu[None], good)[0] == ERR_ARG
            assert _raw(be, [0], [abi.EUCLID2], bad, [0], mu[None], good)[0] == 0  # a row no item names is not read
        assert _raw(be, [0], [abi.EUCLID2], rows2, [-1], mu[None], good)[0] == ERR_ARG
        assert _raw(be, [2], [abi.EUCLID2], rows2, [0], mu[None], good)[0] == ERR_RANGE
        assert _raw(be, [-1], [abi.EUCLID2], rows2, [0], mu[None], good)[0] == ERR_RANGE
        assert _raw(be, [0], [0], rows2, [0], mu[None], good)[0] == ERR_ARG
        assert _raw(be, [0], [6], rows2, [0], mu[None], good)[0] == ERR_ARG
        assert _raw(be, [0], [abi.EUCLID2], rows2, [0], mu[None], good, recs=False)[0] == ERR_ARG
        assert _raw(be, [0], [abi.EUCLID2], rows2, [0], mu[None], bad_opts[0], n=0)[0] == 0  # n = 0: nothing is looked at
        with pytest.raises(iif.NbpError, match="tol"):
            be.run_mixture([0], [abi.EUCLID2], rows2, mu[None], tol=-1.0)
        with pytest.raises(iif.NbpError, match="label"):
            be.kde_mixture(abi.EUCLID2, X, bw, np.full(64, 9), mu)
        with pytest.raises(iif.NbpError):
            be.kde_mixture(abi.EUCLID2, X, bw, lab, mu, max_iter=0)
        # the context stays usable
        recs, _ = be.run_mixture([0], [abi.EUCLID2], rows2, mu[None])
        assert recs[0]["n_comp"] == 2 and np.isfinite(recs[0]["objective"])
    finally:
        be.close()


def _bimodal_graph(n_vars):
    fg = iif.initfg(iif.SolverParams(N=200))
    a, b = np.array([-2.0, 1.0]), np.array([2.0, -1.0])
    A, B = np.array([[0.04, 0.01], [0.01, 0.03]]), np.array([[0.03, -0.01], [-0.01, 0.05]])
    for i in range(n_vars):
        iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
    iif.addFactor(fg, ["x0"], iif.Mixture(iif.Prior, [iif.MvNormal(a, A), iif.MvNormal(b, B)], [0.3, 0.7]))
    for i in range(n_vars - 1):
        iif.addFactor(fg, [f"x{i}", f"x{i + 1}"], iif.LinearRelative(iif.MvNormal([1.0, 0.5], [0.05, 0.05])))
    return fg, (a, A), (b, B)


@pytest.mark.parametrize("n_vars", (1, 3))
def test_session_equals_the_host_copy_and_moves_no_belief(hip_backend, n_vars):
    fg, _, _ = _bimodal_graph(n_vars)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=17)
        before = dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"])
        got = ses.fitBeliefMixtures(tol=0.0, maxIter=10)
        assert dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"]) == before
        host = iif.fitBeliefMixtureAll(fg, tol=0.0, maxIter=10)
        assert list(got) == fg.ls() == list(host)
        for v in fg.ls():
            var = fg.getVariable(v)
            m = var.varType.manifold
            lab, mu = mixture.starting_from_modes(host[v].modes, abi.MIX_MAX)
            assert np.array_equal(got[v].modes.labels, host[v].modes.labels), v
            f64, f80 = xc.restate(m, coords(m, var.val), var.bw, lab, mu, tol=0.0, max_iter=10)
            xc.input_conditions(f64, v)
            assert got[v].n_comp == host[v].n_comp == f64.n_comp >= (2 if n_vars == 1 else 1) and got[v].iters == host[v].iters == 10
            K = f64.n_comp
            for name, dev, a, b in (("weights", got[v].weights, f64.weight[:K], f80.weight[:K]), ("means", got[v].means, f64.mean[:K, :2], f80.mean[:K, :2]),
                                    ("covs", got[v].covs, f64.cov[:K, :2, :2], f80.cov[:K, :2, :2]), ("J", got[v].objective, f64.objective, f80.objective)):
                assert np.all(np.abs(np.asarray(dev) - np.asarray(a, dtype=np.float64)) <= xc.tolerance(a, b)), (v, name, dev, a)
                assert np.array_equal(np.asarray(getattr(host[v], "objective" if name == "J" else name)), np.asarray(a, dtype=np.float64)), (v, name)
            assert np.array_equal(got[v].labels, host[v].labels) and np.array_equal(got[v].counts, host[v].counts), v
        one = ses.fitBeliefMixtures(["x0"], maxComponents=1)
        assert list(one) == ["x0"] and one["x0"].n_comp == 1 and one["x0"].counts.tolist() == [200]
        assert np.all(one["x0"].labels == 0)  # a particle that started in no component is in the one there is after the first E-step
        assert dict(uploads=ses.stats["uploads"], readbacks=ses.stats["readbacks"]) == before


def test_a_mixture_prior_comes_back_out_of_a_solve(hip_backend):
    """the seam: a Euclid(2) variable under Mixture(Prior, [N(a, A), N(b, B)], [0.3, 0.7]), a and b 20 sigma apart, solved at N = 200.
    The bands come from the sampling alone: a component's share of 200 draws has standard deviation sqrt(0.21 / 200), its mean
    sigma / sqrt(n_k) per coordinate; four of each."""
    fg, (a, A), (b, B) = _bimodal_graph(1)
    iif.solveTree(fg, backend=hip_backend, seed=23)
    bm = iif.fitBeliefMixture(fg, "x0", backend=hip_backend)
    print(f"weights {bm.weights}, means {bm.means.tolist()}, counts {bm.counts}, {bm.iters} iterations")
    assert bm.n_comp == 2 and bm.converged and bm.n_dropped == 0
    band = 4.0 * np.sqrt(0.21 / 200.0)
    assert abs(bm.weights[0] - 0.7) <= band and abs(bm.weights[1] - 0.3) <= band, bm.weights
    for k, (mean, cov) in enumerate(((b, B), (a, A))):
        n_k = bm.weights[k] * 200.0
        assert np.all(np.abs(bm.means[k] - mean) <= 4.0 * np.sqrt(np.diag(cov)) / np.sqrt(n_k)), (k, bm.means[k], mean)
    prior = bm.asPrior(iif.ContinuousEuclid(2))
    for (w, mu, L, _), wk, mk, Sk in zip(prior.components(), bm.weights, bm.means, bm.covs):
        assert abs(w - wk) <= 1e-15 and np.array_equal(mu, mk) and np.abs(L @ L.T - Sk).max() <= 1e-12
