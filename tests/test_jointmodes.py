"""Joint hypotheses on the host: the per-cell restatement (jointmodes.factor_mode_likelihood_numpy) against the factor likelihood it
refines, the exact inference on tables (joint_modes_from_tables) against brute force, and the scenes whose answer is known.  The
device leg is test_gpu_jointmodes.py."""
import itertools

import numpy as np
import pytest

import jointmodes_cases as jc
import likelihood_cases as lc
from parity_utils import abi, iif

jm, lik = iif.jointmodes, iif.likelihood
MAXK = abi.MAXK


def _case(name, na, nb, seed):
    rng = np.random.default_rng(seed)
    A, B = lc.clouds(name, na, nb, rng)
    return lc.desc(name), lc.points(name, A), lc.points(name, B), rng


# ---- 1. the table against the factor likelihood ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_one_group_is_the_factor_likelihood_bit_for_bit(name):
    d, A, B, _ = _case(name, 70, 50, 11)
    ll, _ = lik.factor_likelihood_numpy(d, A, B)
    for la, lb in ((None, None), (np.zeros(70, dtype=np.int32), np.zeros(50, dtype=np.int32))):
        t, c = jm.factor_mode_likelihood_numpy(d, A, la, B, lb)
        assert np.float64(t[0, 0]).tobytes() == np.float64(ll).tobytes()
        assert np.isnan(t).sum() == MAXK * MAXK - 1
        assert c[0, 0] == 70 and c[1, 0] == (1 if lc.unary(name) else 50) and c[:, 1:].sum() == 0


@pytest.mark.parametrize("name", list(lc.CASES))
def test_cells_are_the_likelihoods_of_the_sub_clouds_and_recombine(name):
    """cell (k, l) is the factor likelihood of the sub-clouds A[labels_a == k], B[labels_b == l] (another summation tree, the same
    definition: held to restate's tolerance of the sub-cloud run), and with no point left out
    logsumexp_kl(T[k, l] + log(n_k n_l)) - log(n_a n_b) is the loglik of the whole item (held to restate's tolerance of that run)"""
    d, A, B, rng = _case(name, 70, 50, 12)
    la, lb = jc.labels(rng, 70, 2), jc.labels(rng, 50, 3)
    t, c = jm.factor_mode_likelihood_numpy(d, A, la, B, lb)
    cols = 1 if lc.unary(name) else 3
    assert np.array_equal(c[0], np.bincount(la, minlength=MAXK))
    assert np.array_equal(c[1], np.bincount(lb, minlength=MAXK) if cols == 3 else np.eye(MAXK, dtype=int)[0])
    terms = []
    for k in range(MAXK):
        for l in range(MAXK):
            if k >= 2 or l >= cols:
                assert np.isnan(t[k, l])
                continue
            sub = lc.restate(d, A[la == k], None if B is None else B[lb == l])
            if np.isfinite(sub[0]):
                ratio = abs(t[k, l] - sub[0]) / sub[2]
                print(f"{name} T[{k},{l}] {t[k, l]!r} sub-cloud {sub[0]!r} tol {sub[2]:.3e} ratio {ratio:.3f}")
                assert ratio <= 1.0
                terms.append(t[k, l] + np.log(float(c[0, k]) * float(c[1, l])))
            else:
                assert t[k, l] == sub[0]
    whole = lc.restate(d, A, B)
    if np.isfinite(whole[0]):
        got = lik._logsumexp(terms) - np.log(70.0 * (1 if lc.unary(name) else 50))
        print(f"{name} recombined {got!r} loglik {whole[0]!r} tol {whole[2]:.3e} ratio {abs(got - whole[0]) / whole[2]:.3f}")
        assert abs(got - whole[0]) <= whole[2]


def test_special_cells():
    rng = np.random.default_rng(13)
    d = lik.likelihood_desc(abi.F_LINREL, abi.EUCLID1, [(1.0, [1.0], [[0.2]])])
    A, B = rng.normal(0.0, 0.1, (40, 1)), rng.normal(1.0, 0.1, (30, 1))
    # -1 leaves a point out of both roles: the table is that of the clouds without those points
    la, lb = jc.labels(rng, 40, 2, minus=0.3), jc.labels(rng, 30, 2, minus=0.3)
    assert (la < 0).any() and (lb < 0).any()
    t, c = jm.factor_mode_likelihood_numpy(d, A, la, B, lb)
    t2, c2 = jm.factor_mode_likelihood_numpy(d, A[la >= 0], la[la >= 0], B[lb >= 0], lb[lb >= 0])
    assert np.array_equal(c, c2) and c[0].sum() == (la >= 0).sum()
    fin = np.isfinite(t)
    assert np.array_equal(fin, np.isfinite(t2)) and fin.sum() == 4 and np.abs(t[fin] - t2[fin]).max() < 1e-12
    # an empty group in the middle: its row and column are NaN, the others are not
    la, lb = jc.labels(rng, 40, 3, empty=1), jc.labels(rng, 30, 3, empty=1)
    t, c = jm.factor_mode_likelihood_numpy(d, A, la, B, lb)
    assert c[0, 1] == 0 and c[1, 1] == 0 and np.isnan(t[1, :]).all() and np.isnan(t[:, 1]).all()
    assert np.isfinite(t[np.ix_([0, 2], [0, 2])]).all()
    # a unary item has one column, and labels_b is not read
    dp = lc.desc("prior_e1_normal")
    t, c = jm.factor_mode_likelihood_numpy(dp, A, jc.labels(rng, 40, 3), None, np.full(5, 99))
    assert np.isfinite(t[:3, 0]).all() and np.isnan(t[:, 1:]).all() and np.isnan(t[3:, 0]).all() and list(c[1]) == [1] + [0] * 7
    # a Uniform cell outside its support is -inf, the cell inside is finite
    du = lik.likelihood_desc(abi.F_LINREL, abi.EUCLID1, [(1.0, [0.5], [[1.0]], lc.U)])
    Bu = np.concatenate([rng.normal(1.0, 0.05, (15, 1)), rng.normal(9.0, 0.05, (15, 1))])
    t, _ = jm.factor_mode_likelihood_numpy(du, A, None, Bu, np.repeat([0, 1], 15))
    assert np.isfinite(t[0, 0]) and t[0, 1] == -np.inf and abs(t[0, 0]) < 1e-12
    # a Gaussian cell 10^4 sigma off stays finite: one maximum per cell
    Bg = np.concatenate([rng.normal(1.0, 0.1, (15, 1)), rng.normal(1.0 + 1e4 * 0.2, 0.1, (15, 1))])
    t, _ = jm.factor_mode_likelihood_numpy(d, A, None, Bg, np.repeat([0, 1], 15))
    assert np.isfinite(t[0, :2]).all() and t[0, 0] > -2.0 and -5.1e7 < t[0, 1] < -4.9e7
    t80, _ = jm.factor_mode_likelihood_numpy(d, A, None, Bg, np.repeat([0, 1], 15), dtype=np.longdouble)
    assert abs(float(t[0, 1] - t80[0, 1])) <= 1e-9 * abs(float(t80[0, 1]))
    # what the restatement refuses
    with pytest.raises(ValueError, match="label outside"):
        jm.factor_mode_likelihood_numpy(d, A, np.full(40, MAXK), B, None)
    with pytest.raises(ValueError, match="one label per point"):
        jm.factor_mode_likelihood_numpy(d, A, np.zeros(39), B, None)


# ---- 2. the inference on tables against brute force ------------------------------------------------------------------------------------
def _brute(K, terms):
    names = sorted(K, key=iif.ppe._natural)
    scores = {}
    for combo in itertools.product(*[range(K[v]) for v in names]):
        at = dict(zip(names, combo))
        s = 0.0
        for t in terms:
            if isinstance(t, jm.MultihypoTerm):
                with np.errstate(divide="ignore"):
                    s += lik._logsumexp([np.log(p) + tab[tuple(at[v] for v in vs)] for p, (vs, tab) in zip(t.prior, t.items)])
            else:
                s += t[1][tuple(at[v] for v in t[0])]
        scores[combo] = s
    return names, scores


def _hold_to_brute(K, terms, tol=1e-9):
    sol = jm.joint_modes_from_tables(K, terms)
    names, scores = _brute(K, terms)
    unknown = [v for v in names if K[v] > 1]
    assert sol.variables == unknown and list(sol.best) == names
    top = max(scores.values())
    logZ = lik._logsumexp(list(scores.values()))
    assert abs(sol.best_logscore - top) <= tol and abs(sol.logZ - logZ) <= tol
    assert abs(scores[tuple(sol.best[v] for v in names)] - top) <= tol
    assert abs(sol.best_weight - np.exp(top - logZ)) <= tol
    assert len(sol.combos) == len(scores) == len(sol.weights) and np.all(sol.logscores[1:] <= sol.logscores[:-1])
    pos = [names.index(v) for v in unknown]
    for combo, s, w in zip(sol.combos, sol.logscores, sol.weights):
        full = [0] * len(names)
        for p, k in zip(pos, combo):
            full[p] = int(k)
        ref = scores[tuple(full)]
        assert (ref == s or abs(ref - s) <= tol) and abs(np.exp(ref - logZ) - w) <= tol
    assert abs(sol.weights.sum() - 1.0) <= 1e-9
    return sol


def test_inference_on_a_chain_of_twelve_two_state_variables():
    rng = np.random.default_rng(21)
    K = {f"x{i}": 2 for i in range(12)}
    terms = [((f"x{i}", f"x{i + 1}"), rng.normal(0, 3, (2, 2))) for i in range(11)] + [(("x0",), rng.normal(0, 3, 2))]
    sol = _hold_to_brute(K, terms)
    assert len(sol.combos) == 4096


def test_inference_on_a_ring_of_three_with_a_pendant():
    rng = np.random.default_rng(22)
    K = {"a": 2, "b": 3, "c": 2, "p": 4, "u": 1}
    terms = [(("a", "b"), rng.normal(0, 3, (2, 3))), (("b", "c"), rng.normal(0, 3, (3, 2))), (("c", "a"), rng.normal(0, 3, (2, 2))),
             (("c", "p"), rng.normal(0, 3, (2, 4))), (("p", "u"), rng.normal(0, 3, (4, 1)))]
    terms[0][1][1, 2] = -np.inf
    sol = _hold_to_brute(K, terms)
    assert sol.best["u"] == 0 and "u" not in sol.variables


def test_inference_with_a_term_over_three_variables():
    rng = np.random.default_rng(23)
    K = {"x": 2, "l1": 2, "l2": 3, "y": 2}
    mh = jm.MultihypoTerm(np.array([0.3, 0.7]), [(("x", "l1"), rng.normal(0, 3, (2, 2))), (("x", "l2"), rng.normal(0, 3, (2, 3)))])
    _hold_to_brute(K, [mh, (("l1", "y"), rng.normal(0, 3, (2, 2))), (("l2", "y"), rng.normal(0, 3, (3, 2)))])


def test_inference_on_a_chain_of_forty_against_viterbi():
    rng = np.random.default_rng(24)
    n = 40
    K = {f"x{i}": 2 + i % 2 for i in range(n)}
    tabs = [rng.normal(0, 3, (K[f"x{i}"], K[f"x{i + 1}"])) for i in range(n - 1)]
    sol = jm.joint_modes_from_tables(K, [((f"x{i}", f"x{i + 1}"), t) for i, t in enumerate(tabs)])
    assert sol.combos is None and sol.weights is None
    # Viterbi and the forward sum, written by hand
    vit, fwd, back = np.zeros(K["x0"]), np.zeros(K["x0"]), []
    for t in tabs:
        m = vit[:, None] + t
        back.append(m.argmax(axis=0))
        vit = m.max(axis=0)
        f = fwd[:, None] + t
        fwd = f.max(axis=0) + np.log(np.exp(f - f.max(axis=0)).sum(axis=0))
    path = [int(vit.argmax())]
    for b in reversed(back):
        path.append(int(b[path[-1]]))
    path.reverse()
    logZ = fwd.max() + np.log(np.exp(fwd - fwd.max()).sum())
    assert [sol.best[f"x{i}"] for i in range(n)] == path
    assert abs(sol.best_logscore - vit.max()) < 1e-9 and abs(sol.logZ - logZ) < 1e-9
    assert abs(sol.best_weight - np.exp(vit.max() - logZ)) < 1e-12


def test_inference_refuses_a_table_above_the_cap_and_handles_no_support():
    K = {f"v{i}": 8 for i in range(5)}
    hub = [((f"v{i}", f"v{j}"), np.zeros((8, 8))) for i in range(5) for j in range(i + 1, 5)]
    with pytest.raises(ValueError, match=r"v0.*v4.*32768 entries"):
        jm.joint_modes_from_tables(K, hub, cap=4096)
    assert jm.joint_modes_from_tables(K, hub, cap=32768, enumerate_up_to=10).combos is None
    with pytest.raises(ValueError, match="shape"):
        jm.joint_modes_from_tables({"a": 2, "b": 2}, [(("a", "b"), np.zeros((2, 3)))])
    # every score -inf: the convention of hypothesis_weights
    sol = jm.joint_modes_from_tables({"a": 2, "b": 2}, [(("a", "b"), np.full((2, 2), -np.inf))])
    assert sol.best_logscore == -np.inf and sol.logZ == -np.inf and np.isnan(sol.weights).all() and np.isnan(sol.best_weight)
    # a tie is resolved the same way every time
    tie = [(("a", "b"), np.zeros((2, 2)))]
    assert jm.joint_modes_from_tables({"a": 2, "b": 2}, tie).best == jm.joint_modes_from_tables({"a": 2, "b": 2}, tie).best
    # no unknowns at all
    sol = jm.joint_modes_from_tables({"a": 1}, [(("a",), np.array([-2.0]))])
    assert sol.variables == [] and sol.best == {"a": 0} and sol.best_logscore == -2.0 and sol.weights.tolist() == [1.0]


# ---- 3. the scenes ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    fg = jc.ring_graph()
    return fg, iif.jointModes(fg)


def test_ring_scene_picks_the_matching_modes(ring):
    fg, j = ring
    assert j.variables == ["a", "b", "c"] and j.skipped == [] and set(j.modes) == {"a", "b", "c", "u"}
    for v, k in (("a", 2), ("b", 2), ("c", 2), ("u", 1)):
        assert j.modes[v].n_modes == k and j.modes[v].n_unconverged == 0 and j.coverage[v] == 1.0
    for v, where in (("a", 0.0), ("b", 1.0), ("c", 2.0)):
        assert j.best[v] == jc.mode_near(j.modes[v], where) and abs(j.best_points[v][0] - where) < 0.1
    assert j.best["u"] == 0 and abs(j.best_points["u"][0] - 3.0) < 0.1
    ab = j.tables["ab"].tables[0]
    ka, kb = jc.mode_near(j.modes["a"], 0.0), jc.mode_near(j.modes["b"], 1.0)
    print("ab table", ab)
    assert ab.shape == (2, 2) and 0.0 < ab[ka, kb] < 1.0 and -1300 < ab[ka, 1 - kb] < -1000
    assert j.tables["cu"].tables[0].shape == (2, 1)
    print("ring: best weight", j.best_weight, "scores", j.logscores[:3])
    assert j.best_weight > 0.999 and j.logscores[0] - j.logscores[1] > 1000 and len(j.combos) == 8
    assert np.array_equal(j.combos[0], [j.best[v] for v in j.variables]) and j.best_logscore == j.logscores[0]


def test_ring_scene_without_the_anchor_keeps_two_readings():
    """seed jointmodes_cases.RING_SEED; the band was checked on this restatement before it was asserted anywhere else"""
    fg = jc.ring_graph(with_cu=False)
    j = iif.jointModes(fg)
    assert j.variables == ["a", "b", "c"] and "u" not in j.modes
    low = [jc.mode_near(j.modes[v], w) for v, w in (("a", 0.0), ("b", 1.0), ("c", 2.0))]
    high = [1 - k for k in low]
    top = {tuple(c) for c in j.combos[:2]}
    print("two readings", j.combos[:2], j.weights[:3])
    assert top == {tuple(low), tuple(high)}
    assert np.all((j.weights[:2] > 0.4) & (j.weights[:2] < 0.6)) and np.all(j.weights[2:] < 1e-300) and len(j.weights) == 8


def test_multihypo_scene():
    fg = jc.doors_graph()
    j = iif.jointModes(fg)
    assert j.variables == ["x"] and j.modes["x"].n_modes == 2 and j.modes["l1"].n_modes == 1 and j.modes["l2"].n_modes == 1
    assert j.best["x"] == jc.mode_near(j.modes["x"], 2.05) and j.best["l1"] == 0 and j.best["l2"] == 0
    door = j.tables["door"]
    assert door.hypotheses == ["l1", "l2"] and door.hypo_prior.tolist() == [0.5, 0.5]
    assert door.variables == [("x", "l1"), ("x", "l2")] and [t.shape for t in door.tables] == [(2, 1), (2, 1)]
    term = np.array([lik._logsumexp([np.log(0.5) + door.tables[0][k, 0], np.log(0.5) + door.tables[1][k, 0]]) for k in range(2)])
    prior = j.tables["xprior"].tables[0][:, 0]
    order = [int(c[0]) for c in j.combos]
    assert np.abs(j.logscores - (term + prior)[order]).max() < 1e-12
    # the sighting alone cannot tell the doors apart; the prior does
    alone = iif.jointModes(fg, labels=["door"])
    assert abs(alone.logscores[0] - alone.logscores[1]) < 1.0 and j.best_weight > 0.999
    # one factor's tables through the public query, and a factor the query does not support
    one = iif.factorModeLikelihood(fg, "door", modes=j.modes)
    assert all(np.array_equal(a, b) for a, b in zip(one.tables, door.tables)) and one.coverage == door.coverage
    fg.factors["msg"] = iif.factorgraph.DFGFactor("msg", ["x"], iif.factorgraph.MsgPrior(3))
    assert iif.factorModeLikelihoodAll(fg, modes=j.modes).skipped == ["msg"] and iif.jointModes(fg).skipped == ["msg"]
    with pytest.raises(ValueError, match="factor msg:"):
        iif.factorModeLikelihood(fg, "msg")
    # maxModes = 1 keeps the heaviest mode of x only: its other points are left out
    j1 = iif.jointModes(fg, labels=["door", "xprior"], maxModes=1)
    assert j1.variables == [] and j1.coverage["x"] == 40 / 64 and j1.best == {"l1": 0, "l2": 0, "x": 0}
    with pytest.raises(ValueError, match="maxModes"):
        iif.jointModes(fg, maxModes=9)
