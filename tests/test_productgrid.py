"""Local products on a grid (productgrid.py) on the host: the numpy restatement against closed forms, the planner, and the
cross-check with the factor likelihood -- the sum of a message over the points of the variable's own cloud is that factor's
likelihood.  Explicit extents; 1e-12 absolute on logs unless a test says otherwise."""
import math

import numpy as np
import pytest

import likelihood_cases as lc
import productgrid_cases as pgc
from parity_utils import abi, iif

pg = iif.productgrid
lik = iif.likelihood
ATOL = 1e-12


def _normal_logpdf(x, mu, sigma):
    return -0.5 * ((x - mu) / sigma) ** 2 - math.log(sigma) - 0.5 * math.log(2 * math.pi)


def _line_graph(n_other=1, other=0.3, sigma_rel=0.5, seed=3):
    """x with Prior(Normal(0, 1)) and LinearRelative(Normal(1, sigma_rel)) from the neighbour u"""
    fg = iif.initfg(iif.SolverParams(N=max(n_other, 8)))
    rng = np.random.default_rng(seed)
    for v in ("u", "x"):
        iif.addVariable(fg, v, iif.ContinuousScalar)
    pts = np.full((1, 1), other) if n_other == 1 else rng.normal(0.0, 1.0, (n_other, 1))
    iif.setValKDE(fg, "u", pts, [0.1])
    iif.setValKDE(fg, "x", rng.normal(1.0, 0.5, (8, 1)), [0.2])
    iif.addFactor(fg, ["x"], iif.Prior(iif.Normal(0.0, 1.0)), label="xf1")
    iif.addFactor(fg, ["u", "x"], iif.LinearRelative(iif.Normal(1.0, sigma_rel)), label="uxf1")
    return fg


EXT = (-8.0, 16.0 / 256)  # [-8, 8] at n = 257


def test_a_normal_prior_alone_is_its_log_pdf_and_has_mass_one():
    fg = _line_graph()
    r = iif.localProductGrid(fg, "x", n=257, extent=EXT, factors=["xf1"])
    assert r.factors == ["xf1"] and r.skipped == [] and r.logp.shape == (257,)
    err = np.abs(r.logp - _normal_logpdf(r.axes[0], 0.0, 1.0)).max()
    print(f"prior alone: logZ {r.logZ!r}, largest cell error {err:.3e}")
    assert abs(r.logZ) <= ATOL and err <= ATOL
    assert r.argmax == 128 and r.point[0] == 0.0 and r.logmax == r.logp[128]
    assert abs(r.density().sum() * EXT[1] - 1.0) <= ATOL


def test_prior_and_relative_factor_from_a_one_point_neighbour():
    fg = _line_graph()
    r = iif.localProductGrid(fg, "x", n=257, extent=EXT)
    assert r.factors == ["uxf1", "xf1"]
    want = _normal_logpdf(1.3, 0.0, math.sqrt(1.25))
    mean, cov = r.moments()
    print(f"logZ {r.logZ!r} against {want!r}; mean {mean[0]!r}, variance {cov[0, 0]!r}")
    assert abs(r.logZ - want) <= ATOL
    assert abs(mean[0] - 1.04) <= ATOL and abs(cov[0, 0] - 0.2) <= ATOL


def test_the_message_of_a_200_point_neighbour_has_mass_one():
    fg = _line_graph(n_other=200, sigma_rel=0.1)
    r = iif.localProductGrid(fg, "x", n=257, extent=EXT, factors=["uxf1"])
    print(f"message of 200 points: logZ {r.logZ!r}")
    assert abs(r.logZ) <= ATOL


def test_a_uniform_prior_is_flat_inside_and_minus_inf_outside():
    fg = iif.initfg(iif.SolverParams(N=8))
    iif.addVariable(fg, "x", iif.ContinuousScalar)
    iif.addFactor(fg, ["x"], iif.Prior(iif.Uniform(-1.0, 2.0)), label="xf1")
    r = iif.localProductGrid(fg, "x", n=65, extent=(-4.0, 0.125))
    inside = (r.axes[0] >= -1.0) & (r.axes[0] <= 2.0)
    assert np.all(r.logp[~inside] == -np.inf) and np.abs(r.logp[inside] + math.log(3.0)).max() <= ATOL
    assert r.argmax == int(np.flatnonzero(inside)[0])
    # nothing in the support anywhere: the record says so
    r = iif.localProductGrid(fg, "x", n=9, extent=(5.0, 0.125))
    assert np.all(r.logp == -np.inf) and r.logZ == -np.inf and r.logmax == -np.inf and r.argmax == -1 and np.all(np.isnan(r.point))


def test_no_items_is_flat_zero_with_the_volume_as_evidence():
    for man, n, ext in ((abi.EUCLID1, [7], [0.5, 0.25]), (abi.EUCLID2, [5, 4], [0.0, 0.5, -1.0, 0.125]),
                        (abi.SE2, [5, 4, 3], [0.0, 0.5, -1.0, 0.125, -np.pi, 2 * np.pi / 3])):
        logp, logZ, logmax, argmax = iif.product_grid_numpy(man, n, ext, [])
        assert logp.shape == tuple(n) and np.all(logp == 0.0) and logmax == 0.0 and argmax == 0
        assert abs(logZ - sum(math.log(k * s) for k, s in zip(n, ext[1::2]))) <= ATOL
    # an axis of one point is a slice: it adds log 1
    logp, logZ, _, _ = iif.product_grid_numpy(abi.EUCLID2, [6, 1], [0.0, 0.5, 2.0, 0.125], [])
    assert abs(logZ - math.log(6 * 0.5)) <= ATOL


def test_a_multihypo_group_of_two_identical_neighbours_is_the_plain_factor():
    fg = lc.doors_graph()
    iif.setValKDE(fg, "l2", fg.getVal("l1").copy(), [0.05])
    mh = iif.localProductGrid(fg, "x", n=33, extent=(-0.5, 1.0 / 32))
    plain = iif.initfg(iif.SolverParams(N=200))
    for v in ("x", "l1"):
        iif.addVariable(plain, v, iif.ContinuousScalar)
        iif.setValKDE(plain, v, fg.getVal(v).copy(), [0.05])
    iif.addFactor(plain, ["x", "l1"], iif.LinearRelative(iif.Normal(0.0, 0.2)), label="door")
    one = iif.localProductGrid(plain, "x", n=33, extent=(-0.5, 1.0 / 32))
    err = np.abs(mh.logp - one.logp).max()
    print(f"group (0.5, 0.5) against the plain factor: {err:.3e}, |l| up to {np.abs(one.logp).max():.2f}")
    assert np.all(np.isfinite(one.logp)) and err <= 1e-15 and abs(mh.logZ - one.logZ) <= 1e-15
    # a group of one with log_prior 0 is the message untouched, bit for bit
    d = lik.factor_items(plain, "door").descs[0]
    a = iif.product_grid_numpy(abi.EUCLID1, [33], [-0.5, 1.0 / 32], [(d, 0, plain.getVal("l1"), 0, 0.0)])[0]
    assert np.array_equal(a, one.logp)
    assert np.array_equal(a, pg.message_numpy(d, 0, pg.grid_cells(one.axes), plain.getVal("l1")))


def _se2_point(x, y, th):
    return np.array([[x, y, math.cos(th), math.sin(th), -math.sin(th), math.cos(th)]])


@pytest.mark.parametrize("role", [0, 1])
def test_an_se2_relative_factor_peaks_at_the_composed_pose(role):
    u, z = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.5, 0.25])
    if role == 1:  # u (+) z
        th = u[2] + z[2]
        c, s = math.cos(u[2]), math.sin(u[2])
        want = np.array([u[0] + c * z[0] - s * z[1], u[1] + s * z[0] + c * z[1], th])
    else:          # u (-) z: the pose whose composition with z is u
        th = u[2] - z[2]
        c, s = math.cos(th), math.sin(th)
        want = np.array([u[0] - (c * z[0] - s * z[1]), u[1] - (s * z[0] + c * z[1]), th])
    fg = iif.initfg(iif.SolverParams(N=8))
    for v in ("a", "b"):
        iif.addVariable(fg, v, iif.SpecialEuclidean2)
    me, other = ("a", "b") if role == 0 else ("b", "a")
    iif.setValKDE(fg, other, _se2_point(*u), [0.1, 0.1, 0.1])
    iif.addFactor(fg, ["a", "b"], iif.ManifoldFactor(iif.MvNormal(list(z), [0.3, 0.2, 0.1])), label="abf1")
    n, k, step = [9, 7, 5], [4, 2, 3], [0.125, 0.25, 0.0625]
    ext = np.ravel([[want[a] - k[a] * step[a], step[a]] for a in range(3)])
    r = iif.localProductGrid(fg, me, n=n, extent=ext)
    print(f"role {role}: argmax {np.unravel_index(r.argmax, n)}, point {r.point}, wanted {want}")
    assert np.unravel_index(r.argmax, n) == tuple(k) and np.abs(r.point - want).max() < 1e-12
    # the peak is the density's maximum: log N(0) of the measurement model
    assert abs(r.logmax + (1.5 * math.log(2 * math.pi) + math.log(0.3 * 0.2 * 0.1))) < 1e-9


def test_a_fractional_variable_is_skipped_and_refused_when_named():
    fg = lc.doors_graph()
    r = iif.localProductGrid(fg, "l1", n=9, extent=(-1.0, 0.25))
    assert r.skipped == ["door"] and r.factors == [] and np.all(r.logp == 0.0)
    with pytest.raises(ValueError, match="door.*fractional"):
        iif.localProductGrid(fg, "l1", n=9, extent=(-1.0, 0.25), factors=["door"])
    fg.factors["msg"] = iif.factorgraph.DFGFactor("msg", ["x"], iif.factorgraph.MsgPrior(3))
    fg._adj["x"].append("msg")  # (a message prior is put in by hand, as the factor-likelihood tests do: the adjacency with it)
    assert iif.localProductGrid(fg, "x", n=9, extent=(1.0, 0.25)).skipped == ["msg"]
    with pytest.raises(ValueError, match="factor msg"):
        iif.localProductGrid(fg, "x", n=9, extent=(1.0, 0.25), factors=["msg"])
    with pytest.raises(ValueError, match="does not touch"):
        iif.localProductGrid(fg, "l2", n=9, extent=(1.0, 0.25), factors=["msg"])
    every = iif.localProductGridAll(fg, n=9, extent={"x": (1.0, 0.25), "l1": (-1.0, 0.25), "l2": (1.0, 0.25)})
    assert list(every) == ["l1", "l2", "x"] and every["x"].factors == ["door"] and every["l2"].skipped == ["door"]


def test_the_automatic_extent_is_the_marginal_grids():
    rng = np.random.default_rng(5)
    fg = iif.initfg(iif.SolverParams(N=50))
    iif.addVariable(fg, "p", iif.ContinuousEuclid(2))
    iif.setValKDE(fg, "p", rng.normal(0, 1, (50, 2)), [0.3, 0.2])
    iif.addVariable(fg, "s", iif.SpecialEuclidean2)
    iif.setValKDE(fg, "s", pgc.cloud(abi.SE2, 50, rng), [0.3, 0.2, 0.1])
    r = iif.localProductGrid(fg, "p", n=[16, 12], margin=3.0)
    _, axes = iif.marginalGrid(fg, "p", (1, 2), [16, 12], margin=3.0)
    assert np.array_equal(r.axes[0], axes[0]) and np.array_equal(r.axes[1], axes[1])
    r = iif.localProductGrid(fg, "s", n=[8, 6, 4])
    _, axes = iif.marginalGrid(fg, "s", (1, 2), [8, 6])
    _, th = iif.marginalGrid(fg, "s", (3,), [4])
    assert np.array_equal(r.axes[0], axes[0]) and np.array_equal(r.axes[1], axes[1]) and np.array_equal(r.axes[2], th[0])


def test_marginal_and_density_integrate_to_one():
    rng = np.random.default_rng(6)
    items = pgc.items_for([("linrel_e2_full", 1), ("prior_e2_mix2", 0)], [40, 0], rng)
    n, ext = [48, 40], pgc.extent_for(abi.EUCLID2, [48, 40], -6.0, 7.0)
    logp, logZ, logmax, argmax = iif.product_grid_numpy(abi.EUCLID2, n, ext, items)
    r = pg._result(abi.EUCLID2, n, logp, (logZ, logmax, argmax), ext, [], [])
    assert abs(r.density().sum() * ext[1] * ext[3] - 1.0) < 1e-12
    m1, m2, m21 = r.marginal(1), r.marginal(2), r.marginal((2, 1))
    assert m1.shape == (48,) and m2.shape == (40,) and m21.shape == (40, 48)
    assert abs(np.exp(m1).sum() * ext[1] - 1.0) < 1e-12 and abs(np.exp(m2).sum() * ext[3] - 1.0) < 1e-12
    assert np.allclose(m21.T, r.logp - r.logZ, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name,role", pgc.ITEM_CASES, ids=[f"{n}-role{r}" for n, r in pgc.ITEM_CASES])
def test_the_message_summed_over_the_variables_cloud_is_the_factor_likelihood(name, role):
    """N one-cell grids at the points of the variable's own cloud: logsumexp_i(logp_i) - log n is factor_likelihood_numpy's loglik,
    within the tolerance likelihood_cases works out for the case"""
    rng = np.random.default_rng(900 + sum(map(ord, name)))
    A, B = lc.clouds(name, 24, 17, rng)
    d, m = lc.desc(name), lc.CASES[name][1]
    l64, _, tol, _ = lc.restate(d, lc.points(name, A), lc.points(name, B))
    mine, other = (A, lc.points(name, B)) if role == 0 else (B, lc.points(name, A))
    ones = [1] * abi.MANIFOLD_DIM[m]
    cells = np.array([iif.product_grid_numpy(m, ones, np.ravel([[x, 1.0] for x in p]), [(d, role, other, 0, 0.0)])[0].reshape(())
                      for p in mine])
    mx = cells.max()
    got = mx + math.log(np.exp(cells - mx).sum()) - math.log(len(cells)) if mx > -np.inf else -np.inf
    print(f"{name} role {role}: from the cells {got!r}, factor likelihood {l64!r}, tolerance {tol:.3e}")
    assert (got == l64) if not np.isfinite(l64) else abs(got - l64) <= tol
