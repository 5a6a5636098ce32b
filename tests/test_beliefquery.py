"""Belief queries on the CPU: the numpy restatement of the definitions (incrementalinference.jl_amd/beliefquery.py) against
closed forms, and the mirror's names on solves with the oracle backend -- among them the reference's own assertions where the
restated graphs meet them.  The device side is tests/test_gpu_beliefquery.py."""
import math

import numpy as np
import pytest

import band_cases
import ppe_cases as pc
import query_cases as qc
from parity_utils import abi, iif

bq = iif.beliefquery


@pytest.mark.parametrize("man", qc.MANIFOLDS)
def test_one_point_belief_is_the_gaussian_pdf_of_the_offset(man):
    """points and offsets on a binary grid, so that the offset the density sees, (x + off) - x, is the offset itself"""
    rng = np.random.default_rng(man)
    D, bw = abi.MANIFOLD_DIM[man], pc.hand_bandwidth(man)
    for _ in range(40):
        x = rng.integers(-8, 9, (1, D)) / 8.0
        off = rng.integers(-64, 65, D) / 64.0
        want = qc.gauss_pdf(off, bw)
        got = bq.density_numpy(man, x, bw, x + off)[0]
        assert abs(got - want) <= 1e-15 * want, (got, want)


def test_two_one_point_beliefs_give_the_closed_form_mmd():
    for man in qc.MANIFOLDS:
        D = abi.MANIFOLD_DIM[man]
        for sigma in (0.001, 1.0):
            for d in (0.0, 0.125, 1.0, 2.5):
                b = np.zeros((1, D))
                b[0, 0] = d
                want = qc.mmd_two_points(d, sigma)
                got = bq.mmd_numpy(man, np.zeros((1, D)), b, sigma)
                assert abs(got - want) <= 1e-15 * want, (man, sigma, d, got, want)


def test_density_of_a_line_belief_integrates_to_one():
    rng = np.random.default_rng(1)
    X = pc.cloud("two_cluster", abi.EUCLID1, 80, rng)
    h = 0.15
    grid = np.linspace(X.min() - 10 * h, X.max() + 10 * h, 4001)
    p = bq.density_numpy(abi.EUCLID1, X, [h], grid[:, None])
    area = float(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(grid)))
    assert abs(area - 1.0) < 1e-6, area


def test_circle_wraps_the_offset():
    h = 0.2
    got = bq.density_numpy(abi.CIRCULAR, [[3.1]], [h], [[-3.1]])[0]
    want = qc.gauss_pdf(2 * math.pi - 6.2, h)
    assert abs(got - want) <= 1e-13 * want, (got, want)  # (the wrapped offset carries the rounding of 6.2 - 2 pi: ~1e-15 / h^2 * 0.08)
    # and without the wrap it would be the pdf at 6.2: nothing
    assert bq.density_numpy(abi.EUCLID1, [[3.1]], [h], [[-3.1]])[0] < 1e-200
    # SE(2): the heading wraps, x and y do not
    bw = np.array([0.3, 0.4, h])
    got = bq.density_numpy(abi.SE2, [[0.0, 0.0, 3.1]], bw, [[0.0, 0.0, -3.1]])[0]
    assert abs(got - want * qc.gauss_pdf(0, 0.3) * qc.gauss_pdf(0, 0.4)) <= 1e-13 * got


def test_bad_bandwidth_gives_nan():
    X = pc.cloud("gaussian", abi.EUCLID2, 20, np.random.default_rng(2))
    for bw in ([0.0, 0.3], [0.3, np.nan], [np.inf, 0.3], [-1.0, 0.3]):
        assert np.isnan(bq.density_numpy(abi.EUCLID2, X, bw, X[:3])).all()


@pytest.mark.parametrize("man", qc.MANIFOLDS)
def test_mmd_of_a_belief_with_itself_is_zero_and_mmd_is_symmetric(man):
    rng = np.random.default_rng(20 + man)
    A, B = pc.cloud("gaussian", man, 150, rng), pc.cloud("across_pi", man, 73, rng)
    for sigma in (0.001, 1.0):
        assert bq.mmd_numpy(man, A, A, sigma) == 0.0
        assert bq.mmd_numpy(man, A, A.copy(), sigma) == 0.0
        ab, ba = bq.mmd_numpy(man, A, B, sigma), bq.mmd_numpy(man, B, A, sigma)
        assert abs(ab - ba) <= 1e-15, (ab, ba)
        assert ab > 0


def test_mmd_grows_with_the_shift_of_a_normal():
    rng = np.random.default_rng(3)
    a, z = rng.normal(0, 1, (10000, 1)), rng.normal(0, 1, (10000, 1))
    for sigma in (0.001, 1.0):
        v = [bq.mmd_numpy(abi.EUCLID1, a, z + delta, sigma) for delta in (0.0, 0.5, 2.0)]
        print(f"sigma {sigma}: mmd at shifts 0, 0.5, 2 = {v}")
        assert v[0] < v[1] < v[2], v


def test_se2_heading_enters_with_weight_one():
    a, b = np.array([[0.0, 0.0, 0.3]]), np.array([[0.0, 0.0, 1.0]])
    assert bq.SE2_HEADING_WEIGHT == 1.0
    assert abs(bq.mmd_numpy(abi.SE2, a, b, 1.0) - qc.mmd_two_points(0.7, 1.0)) <= 1e-15


def test_mirror_on_a_solved_chain_with_the_oracle_backend(oracle_backend):
    fg, fg2 = qc.chain6(5), qc.chain6(5)
    iif.solveTree(fg, backend=oracle_backend, seed=71)
    iif.solveTree(fg2, backend=oracle_backend, seed=72)
    b = iif.getBelief(fg, "x5")
    v = fg.getVariable("x5")
    assert b.manifold == abi.EUCLID1 and np.array_equal(b.pts, v.val) and np.array_equal(b.bw, v.bw)
    pts = np.array([[4.0], [5.0], [5.3], [9.0]])
    for be in (None, oracle_backend):  # the oracle has no such entry point: numpy serves
        got = b(pts, backend=be)
        assert np.array_equal(got, bq.density_numpy(abi.EUCLID1, v.val, v.bw, pts))
    assert b(pts)[1] > b(pts)[0] > b(pts)[3] and b(pts)[3] < 1e-12
    assert np.array_equal(b([5.0]), b(pts)[1:2]) and np.array_equal(b(5.0), b(pts)[1:2])  # a single point
    labels, vals = iif.mmdVariables(fg, fg2, backend=oracle_backend)
    assert labels == [f"x{i}" for i in range(6)]
    for i, l in enumerate(labels):
        assert vals[i] == bq.mmd_numpy(abi.EUCLID1, fg.getVal(l), fg2.getVal(l), 0.001)
        assert vals[i] == iif.mmd(iif.getBelief(fg, l), fg2.getVal(l), iif.ContinuousScalar)
        assert 0 < vals[i] < 1e-4, vals  # two solves of one graph: close, and not the same particles
    labels, same = iif.mmdVariables(fg, fg, labels=["x5", "x0"])
    assert labels == ["x5", "x0"] and np.all(same == 0.0)
    assert iif.isapproxBeliefs(iif.getBelief(fg, "x5"), iif.getBelief(fg, "x5"), iif.ContinuousScalar)
    assert not iif.isapproxBeliefs(iif.getBelief(fg, "x5"), iif.getBelief(fg, "x0"), iif.ContinuousScalar)  # 5 apart: 2.5e-2


def test_reference_assertion_multihypo_and_chain_mmd(oracle_backend, monkeypatch):
    """test/testMultihypoAndChain.jl:78-84 on tests/band_cases.py's restatement of that graph (its seeds, the oracle backend):
    `mmd(manikde!(2 .+ 0.1 randn), getBelief(fg, :l2), ContinuousScalar) < 1e-3`"""
    got = {}
    solve = iif.solveTree

    def keep(fg, *a, **k):
        got["fg"] = fg
        return solve(fg, *a, **k)

    monkeypatch.setattr(band_cases.iif, "solveTree", keep)
    band_cases.case_multihypo_and_chain(oracle_backend)
    monkeypatch.undo()
    L2 = iif.getBelief(got["fg"], "l2")
    pts = 2.0 + 0.1 * np.random.default_rng(96).normal(size=(len(L2.pts), 1))
    value = iif.mmd(pts, L2, iif.ContinuousScalar)
    print(f"mmd(N(2, 0.1) samples, l2) = {value:.6e}")
    assert value < 1e-3, value


def test_reference_assertion_three_door_sighting_density(oracle_backend):
    """test/testMultiHypo3Door.jl:77-99: the sighting's convolution to x0 has a peak at each of the four doors,
    `0.1 < X0([l0])[1]` ... (tests/band_cases.py does not hold that graph; tests/three_door_cases.py does, and this is its first
    part with its seeds)"""
    import three_door_cases as td
    fg = iif.initfg(iif.SolverParams(N=200))
    for k, pos in enumerate(td.L):
        iif.addVariable(fg, f"l{k}", iif.ContinuousScalar)
        iif.addFactor(fg, [f"l{k}"], iif.Prior(iif.Normal(pos, 0.01)))
    iif.initAll(fg, backend=oracle_backend, seed=40)
    iif.addVariable(fg, "x0", iif.ContinuousScalar)
    f1 = iif.addFactor(fg, ["x0", "l0", "l1", "l2", "l3"], iif.LinearRelative(iif.Normal(0.0, 0.25)), multihypo=td.MH)
    pts, bw = iif.approxConvBelief(fg, f1.label if hasattr(f1, "label") else f1, "x0", backend=oracle_backend, seed=41)
    X0 = iif.Belief(iif.ContinuousScalar, pts, bw)
    dens = [X0([x])[0] for x in td.L]
    print(f"X0 at the doors: {dens}")
    for d in dens:
        assert 0.1 < d, dens


# ---- which backend a graph-level query uses, what it writes to it, and who closes it ---------------------------------------------
class _Recorder:
    """a stand-in backend that records what the graph-level functions do to it; `has`: the run_* methods it offers; `fail`: they raise"""
    made = []

    def __init__(self, N, n_slots, side_ints=0, has=("run_meancov", "run_modes", "run_mmd"), fail=False):
        self.N, self.n_slots, self.writes, self.closed, self.fail = N, n_slots, [], 0, fail
        for m in has:
            setattr(self, m, getattr(self, "_" + m))
        _Recorder.made.append(self)

    def slot_write(self, *a):
        raise AssertionError("the graph-level queries write beliefs in one batch")

    def beliefs_write(self, slots, manifolds, beliefs):
        assert len(slots) == len(manifolds) == len(beliefs)
        self.writes.append(list(slots))

    def close(self):
        self.closed += 1

    def _ran(self):
        if self.fail:
            raise RuntimeError("the launch failed")

    def _run_meancov(self, slots, manifolds):
        self._ran()
        return np.zeros((len(slots), abi.MAXD)), np.zeros((len(slots), abi.MAXD, abi.MAXD))

    def _run_modes(self, slots, manifolds, **kw):
        self._ran()
        n = len(slots)
        z = np.zeros(n, dtype=np.int32)
        return (np.zeros((n, abi.MODES_MAX), dtype=iif.HipBackend._MODE_REC), z, np.zeros((n, self.N), dtype=np.int32),
                np.zeros((n, self.N), dtype=np.int32), z)

    def _run_mmd(self, slots_a, slots_b, manifolds, sigma):
        self._ran()
        return np.zeros(len(slots_a))


def _three_variables(seed):
    fg = iif.initfg(iif.SolverParams(N=20))
    rng = np.random.default_rng(seed)
    for i in range(3):
        iif.addVariable(fg, f"x{i}", iif.ContinuousScalar)
        v = fg.getVariable(f"x{i}")
        v.val, v.bw = rng.normal(i, 0.3, size=(20, 1)), np.array([0.2])
    return fg


_QUERIES = {
    "calcMeanCovarAll": (lambda fg, be: iif.calcMeanCovarAll(fg, backend=be), [0, 1, 2]),
    "getBeliefModesAll": (lambda fg, be: iif.getBeliefModesAll(fg, backend=be), [0, 1, 2]),
    "mmdVariables": (lambda fg, be: iif.mmdVariables(fg, _three_variables(2), backend=be), [0, 1, 2, 3, 4, 5]),
}


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return _same(vars(a), vars(b)) if hasattr(a, "__dict__") else a == b


@pytest.mark.parametrize("name", sorted(_QUERIES))
def test_graph_queries_make_write_and_close_their_backend_once(name):
    query, slots = _QUERIES[name]
    fg = _three_variables(1)
    # a backend passed as a class (or factory): made once, one batch write of slots 0 .. L-1, closed exactly once -- also when the run raises
    for fail in (False, True):
        _Recorder.made = []
        make = lambda N, n_slots, side_ints=0: _Recorder(N, n_slots, side_ints, fail=fail)  # noqa: E731
        if fail:
            with pytest.raises(RuntimeError, match="the launch failed"):
                query(fg, make)
        else:
            query(fg, make)
        (be,) = _Recorder.made
        assert be.writes == [slots] and be.closed == 1 and be.n_slots == len(slots), (fail, be.writes, be.closed)
    _Recorder.made = []
    query(fg, _Recorder)
    assert len(_Recorder.made) == 1 and _Recorder.made[0].writes == [slots] and _Recorder.made[0].closed == 1
    # a backend passed as an instance is never closed
    for fail in (False, True):
        be = _Recorder(20, 6, fail=fail)
        if fail:
            with pytest.raises(RuntimeError, match="the launch failed"):
                query(fg, be)
        else:
            query(fg, be)
        assert be.writes == [slots] and be.closed == 0
    # a backend without the method: the numpy result, nothing written; closed if it was made for the call
    want = query(fg, None)
    _Recorder.made = []
    got = query(fg, lambda N, n_slots, side_ints=0: _Recorder(N, n_slots, side_ints, has=()))
    (be,) = _Recorder.made
    assert _same(got, want) and be.writes == [] and be.closed == 1
    be = _Recorder(20, 6, has=())
    assert _same(query(fg, be), want) and be.writes == [] and be.closed == 0
