"""Belief overlaps on the host (-m "not gpu"): the numpy restatements of incrementalinference.jl_amd/overlap.py against hand values,
quadrature and their own properties; the search against plain brute force; findVariablesNear and findBeliefsNear; the layout of the
new ABI structs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import overlap_cases as oc
import ppe_cases as pc
from parity_utils import abi, iif

ov = iif.overlap
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- hand values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", oc.ADMISSIBLE, ids=lambda s: f"m{s[0]}k{s[1]}")
def test_one_point_each_has_a_closed_form(a, b):
    """n = m = 1: c = prod_k sqrt(2 h_a h_b / (h_a^2 + h_b^2)) exp(-delta_k^2 / (2 s_k)), the differences wrapped across +-pi.
    Both sides are a dozen float64 operations on values below 30 in magnitude: 1e-13 is two orders above their rounding."""
    (ma, ka), (mb, kb) = a, b
    A, B = np.array([[3.0, -0.7, 3.1]])[:, :abi.MANIFOLD_DIM[ma]], np.array([[-2.9, 0.4, -3.0]])[:, :abi.MANIFOLD_DIM[mb]]
    ha, hb = oc.bandwidth(ma), oc.bandwidth(mb, 1.7)
    logc, lab, laa, lbb = ov.overlap_numpy(ma, A, ha, ka, mb, B, hb, kb)
    want = 0.0
    for da, db, circ in zip(ov.mask_coords(ma, ka), ov.mask_coords(mb, kb), ov.mask_kinds(ma, ka)):
        delta = A[0, da] - B[0, db]
        if circ:
            delta = pc.wrap(delta)
            assert abs(delta) < 0.5  # (3.0 against -2.9, 3.1 against -3.0: across the seam)
        s = ha[da] ** 2 + hb[db] ** 2
        want += 0.5 * math.log(2 * ha[da] * hb[db] / s) - delta ** 2 / (2 * s)
    print(f"logc {logc!r} closed form {want!r}")
    assert abs(logc - want) <= 1e-13
    # the self terms of one point: L_aa = -sum_k 1/2 log(2 pi 2 h^2)
    assert abs(laa + sum(0.5 * math.log(4 * math.pi * ha[d] ** 2) for d in ov.mask_coords(ma, ka))) <= 1e-13
    assert math.exp(logc) <= 1.0


# ---- exp(L_ab) against quadrature ------------------------------------------------------------------------------------------------------
def _grid(lo, hi, step):
    return lo + step * np.arange(int(round((hi - lo) / step)) + 1)


@pytest.mark.parametrize("manifold,mask", [(abi.EUCLID1, 1), (abi.EUCLID3, 2), (abi.EUCLID2, 3), (abi.SE2, 3)])
def test_cross_term_is_the_integral_of_the_product_of_the_marginals(manifold, mask):
    """exp(L_ab) = int p_a,K p_b,K on Euclidean coordinates: the trapezoid rule on a grid over both supports, at a step and at half
    of it; the tolerance is 16 x the change between the two, plus 1e-12 of the value for the float64 products behind either side."""
    rng = np.random.default_rng(3)
    A, B = oc.cloud("bimodal", manifold, 30, rng), oc.cloud("gaussian", manifold, 40, rng, 0.4)
    ha, hb = oc.bandwidth(manifold, 0.8), oc.bandwidth(manifold, 1.1)
    dims = ov.mask_coords(manifold, mask)
    lab = float(ov.overlap_numpy(manifold, A, ha, mask, manifold, B, hb, mask)[1])
    vals = []
    for step in (0.3, 0.15):
        axes = [_grid(min(A[:, d].min(), B[:, d].min()) - 3.0, max(A[:, d].max(), B[:, d].max()) + 3.0, step) for d in dims]
        Q = np.zeros((int(np.prod([len(a) for a in axes])), abi.MANIFOLD_DIM[manifold]))
        for d, col in zip(dims, np.meshgrid(*axes, indexing="ij")):
            Q[:, d] = col.reshape(-1)
        p = iif.marginal_density_numpy(manifold, A, ha, dims, Q) * iif.marginal_density_numpy(manifold, B, hb, dims, Q)
        vals.append(math.fsum(p.tolist()) * step ** len(dims))  # (the integrand is below 1e-20 of its peak at the border)
    tol = 16 * abs(vals[0] - vals[1]) + 1e-12 * vals[1]
    print(f"exp(L_ab) {math.exp(lab)!r} quadrature {vals[0]!r} (step 0.3) {vals[1]!r} (step 0.15) tolerance {tol:.3e}")
    assert abs(math.exp(lab) - vals[1]) <= tol


# ---- properties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("manifold", oc.MANIFOLDS)
@pytest.mark.parametrize("kind", oc.CLOUDS)
def test_properties_of_the_coefficient(manifold, kind):
    rng = np.random.default_rng(11)
    full = (1 << abi.MANIFOLD_DIM[manifold]) - 1
    A, B = oc.cloud(kind, manifold, 70, rng), oc.cloud("gaussian", manifold, 45, rng, 0.5)
    ha, hb = oc.bandwidth(manifold), oc.bandwidth(manifold, 0.6)
    same = ov.overlap_numpy(manifold, A, ha, full, manifold, A.copy(), ha.copy(), full)
    assert same[0] == 0.0 and same[1] == same[2] == same[3]
    ab = ov.overlap_numpy(manifold, A, ha, full, manifold, B, hb, full)
    ba = ov.overlap_numpy(manifold, B, hb, full, manifold, A, ha, full)
    ab80 = ov.overlap_numpy(manifold, A, ha, full, manifold, B, hb, full, dtype=np.longdouble)
    noise = max(abs(float(ab[0] - ab80[0])), 4 * np.spacing(max(1.0, abs(float(ab[0])))))
    print(f"logc(a, b) {ab[0]!r} logc(b, a) {ba[0]!r} long-double noise {noise:.3e}")
    assert abs(ab[0] - ba[0]) <= 16 * noise and ab[2] == ba[3] and ab[3] == ba[2]
    assert np.isfinite(ab[0])
    if not pc.circular_coords(manifold):
        assert ab[0] <= 16 * noise  # c <= 1 (Cauchy-Schwarz), up to the rounding of the three terms
    if kind == "far" and manifold != abi.CIRCULAR:  # (nothing on the circle is further than pi away)
        assert -3e6 < ab[0] < -1e5  # 10^3 bandwidths apart: every density underflows, the logarithm does not
    for bad in (0.0, -1.0, np.inf, np.nan):
        hx = ha.copy()
        hx[-1] = bad
        assert all(np.isnan(v) for v in ov.overlap_numpy(manifold, A, hx, full, manifold, B, hb, full))
        assert all(np.isnan(v) for v in ov.overlap_numpy(manifold, B, hb, full, manifold, A, hx, full))
    if abi.MANIFOLD_DIM[manifold] > 1:  # an entry outside the mask is not read
        hx = ha.copy()
        hx[-1] = 0.0
        assert np.isfinite(ov.overlap_numpy(manifold, A, hx, 1, manifold, B, hb, 1)[0])


def test_inadmissible_pairs_and_masks_are_refused():
    X1, X2, X3 = np.zeros((4, 1)), np.zeros((4, 2)), np.zeros((4, 3))
    with pytest.raises(ValueError, match="inadmissible"):
        ov.overlap_numpy(abi.EUCLID1, X1, [1.0], 1, abi.CIRCULAR, X1, [1.0], 1)
    with pytest.raises(ValueError, match="inadmissible"):
        ov.overlap_numpy(abi.SE2, X3, [1.0] * 3, 7, abi.EUCLID3, X3, [1.0] * 3, 7)
    with pytest.raises(ValueError, match="inadmissible"):
        ov.overlap_numpy(abi.EUCLID2, X2, [1.0] * 2, 3, abi.EUCLID2, X2, [1.0] * 2, 1)
    with pytest.raises(ValueError, match="empty mask"):
        ov.overlap_numpy(abi.EUCLID2, X2, [1.0] * 2, 0, abi.EUCLID2, X2, [1.0] * 2, 3)
    with pytest.raises(ValueError, match="outside the manifold"):
        ov.overlap_numpy(abi.EUCLID2, X2, [1.0] * 2, 4, abi.EUCLID2, X2, [1.0] * 2, 3)
    assert ov.admissible(abi.SE2, 3, abi.EUCLID2, 3) and ov.admissible(abi.SE2, 4, abi.CIRCULAR, 1)
    assert ov.dims_mask(abi.SE2, (1, 2)) == 3 and ov.dims_mask(abi.EUCLID3) == 7
    with pytest.raises(ValueError):
        ov.dims_mask(abi.EUCLID2, (3,))
    assert len(oc.ADMISSIBLE) == 99


# ---- the search against plain brute force ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    rng = np.random.default_rng(21)
    line = [(abi.EUCLID2, rng.normal([0.7 * i, 0.0], 0.25, (40, 2)), np.array([0.12, 0.12]), 3) for i in range(14)]
    line[5] = (abi.EUCLID2, line[5][1], np.array([0.12, 0.0]), 3)  # an unusable bandwidth
    mixed = oc.poses_and_landmarks(n=30)[::4]
    return {"line": line, "clusters": oc.clusters(k=3, n=30), "mixed": mixed, "circular": oc.circular_beliefs(V=9, n=30)}


@pytest.mark.parametrize("name", ["line", "clusters", "mixed", "circular"])
def test_search_restatement_equals_plain_brute_force(scenes, name):
    scene, topk = scenes[name], 3
    V = len(scene)
    got = ov.overlap_search_numpy(scene, topk=topk)
    full = ov.overlap_search_numpy(scene, topk=topk, prune=False)
    # plain brute force, pair by pair through the pair form
    logc = np.full((V, V), np.nan)
    for i in range(V):
        for j in range(i + 1, V):
            logc[i, j] = logc[j, i] = float(ov.overlap_numpy(*scene[i], *scene[j])[0])
    valid = [bool(np.all(np.isfinite(s[2][ov.mask_coords(s[0], s[3])]) & (s[2][ov.mask_coords(s[0], s[3])] > 0))) for s in scene]
    logmin, n_pruned = math.log(ov.MIN_COEFF), 0
    for i in range(V):
        if not valid[i]:
            assert got[2][i] == -1 and got[3][i] == 0 and np.all(got[0][i] == -1) and np.all(np.isneginf(got[1][i]))
            continue
        cands = [(j, logc[i, j]) for j in range(V) if j != i and valid[j]]
        idx, val, found = ov.rank_row(cands, topk, logmin)
        assert np.array_equal(got[0][i], idx) and got[1][i].tobytes() == val.tobytes() and got[2][i] == found, (name, i)
        assert np.array_equal(full[0][i], idx) and full[1][i].tobytes() == val.tobytes() and full[3][i] == len(cands)
        assert got[3][i] <= len(cands)
    # the soundness bound on every pruned pair: c <= sqrt(n m) exp(-reach^2 / 2), far below the threshold
    parts = [ov._masked(*s, np.float64) for s in scene]
    for i in range(V):
        for j in range(i + 1, V):
            if valid[i] and valid[j] and ov.box_skips(parts[i][0].min(axis=0), parts[i][0].max(axis=0), parts[i][1], parts[j][0].min(axis=0),
                                                       parts[j][0].max(axis=0), parts[j][1], parts[i][2], ov.REACH):
                n_pruned += 1
                bound = 0.5 * math.log(len(scene[i][1]) * len(scene[j][1])) - 0.5 * ov.REACH ** 2
                assert logc[i, j] <= bound < logmin - 1.0, (name, i, j, logc[i, j], bound)
    print(f"{name}: {V} beliefs, {n_pruned} pairs pruned, evaluated per row {got[3].tolist()}")
    if name == "circular":
        assert n_pruned == 0 and all(got[3][i] == V - 1 for i in range(V))
    if name in ("line", "clusters"):
        assert n_pruned > 0
    if name == "clusters":  # rows with 0, k - 1, k and k + 1 partners; the copies tie and the lower index goes first
        assert sorted(set(got[2].tolist())) == [0, topk - 1, topk, topk + 1]


def test_search_options_that_break_the_soundness_rule_are_refused(scenes):
    line = scenes["line"]
    for kw in ({"reach": 2.0}, {"min_coeff": 1e-9}, {"topk": 0}, {"topk": 17}, {"reach": -1.0}, {"min_coeff": 0.0}, {"N": 10 ** 7}):
        with pytest.raises(ValueError):
            ov.overlap_search_numpy(line, **kw)
    # the rule itself, at its edge for N = 200
    edge = math.exp(math.log(200.0) - 0.5 * 36.0 + 1.0)
    ov.check_search_options(8, edge * 1.0001, 6.0, 200)
    with pytest.raises(ValueError):
        ov.check_search_options(8, edge * 0.9999, 6.0, 200)
    with pytest.raises(ValueError, match="not admissible"):
        ov.overlap_search_numpy(line[:2] + [(abi.CIRCULAR, np.zeros((3, 1)), [0.1], 1)])


# ---- findVariablesNear and findBeliefsNear -----------------------------------------------------------------------------------------------
def test_find_variables_near_on_a_hand_ranked_chain():
    rng = np.random.default_rng(31)
    fg = iif.initfg(iif.SolverParams(N=50))
    for i in range(12):
        iif.addVariable(fg, f"x{i}", iif.ContinuousEuclid(2))
        iif.setValKDE(fg, f"x{i}", rng.normal([float(i), 0.0], 0.01, (50, 2)), [0.05, 0.05])
    iif.addVariable(fg, "l1", iif.ContinuousScalar)
    iif.setValKDE(fg, "l1", rng.normal(2.7, 0.01, (50, 1)), [0.05])
    labels, dist = iif.findVariablesNear(fg, [2.2, 0.0])
    assert labels == ["x2", "l1", "x3"]  # l1's estimate is padded with a zero, as getPPESuggestedAll lays it out: (2.7, 0)
    sug = np.array([np.r_[iif.getPPESuggested(fg, v), 0.0][:2] for v in labels])
    assert np.array_equal(dist, np.sqrt(((sug - [2.2, 0.0]) ** 2).sum(axis=1))) and np.all(np.abs(dist - [0.2, 0.5, 0.8]) < 0.02)
    labels, dist = iif.findVariablesNear(fg, [2.2, 0.0], "^x", number=4)
    assert labels == ["x2", "x3", "x1", "x4"] and np.all(np.diff(dist) >= 0)
    labels, _ = iif.findVariablesNear(fg, [10.2], "^x1", number=2)  # one coordinate of loc: the first coordinate decides
    assert labels == ["x10", "x11"]
    assert iif.findVariablesNear(fg, [0.0, 0.0], "nothing")[0] == []


def test_point_estimates_and_beliefs_rank_a_two_door_scene_differently():
    """`a` believes in two doors, at -1 and +1 on the circle: its mean lies between them, at 0.  Asked what is near +1, the
    reference's ranking puts `b` (at 0.4) before it; the beliefs put `a` first."""
    rng = np.random.default_rng(32)
    fg = iif.initfg(iif.SolverParams(N=100))
    clouds = {"a": np.r_[rng.normal(-1.0, 0.05, 50), rng.normal(1.0, 0.05, 50)], "b": rng.normal(0.4, 0.05, 100), "c": rng.normal(2.5, 0.05, 100)}
    for v, x in clouds.items():
        iif.addVariable(fg, v, iif.Circular)
        iif.setValKDE(fg, v, x.reshape(-1, 1), [0.05])
    labels, dist = iif.findVariablesNear(fg, [1.0])
    assert labels == ["b", "a", "c"] and abs(dist[1] - 1.0) < 0.05
    labels, dens = iif.findBeliefsNear(fg, [1.0])
    assert labels == ["a", "b", "c"] and dens[0] > 1.0 > 1e-3 > dens[1] > dens[2] >= 0.0
    want = iif.marginal_density_numpy(abi.CIRCULAR, clouds["a"].reshape(-1, 1), [0.05], [0], [[1.0]])[0]
    assert dens[0] == want
    assert iif.findBeliefsNear(fg, [1.0], number=1, regexFilter="[bc]")[0] == ["b"]
    with pytest.raises(ValueError):
        iif.findBeliefsNear(fg, [1.0, 2.0], dims=(1,))


def test_find_beliefs_near_mixes_poses_and_landmarks_on_named_coordinates():
    rng = np.random.default_rng(33)
    fg = iif.initfg(iif.SolverParams(N=40))
    iif.addVariable(fg, "x0", iif.SpecialEuclidean2)
    X = np.c_[rng.normal([1.0, 2.0], 0.05, (40, 2)), rng.uniform(-np.pi, np.pi, 40)]
    iif.setValKDE(fg, "x0", pc.to_points(abi.SE2, X), [0.05, 0.05, 0.3])
    iif.addVariable(fg, "l0", iif.ContinuousEuclid(2))
    iif.setValKDE(fg, "l0", rng.normal([1.3, 2.0], 0.05, (40, 2)), [0.05, 0.05])
    iif.addVariable(fg, "s0", iif.ContinuousScalar)  # has no second coordinate: left out
    iif.setValKDE(fg, "s0", rng.normal(1.3, 0.05, (40, 1)), [0.05])
    labels, dens = iif.findBeliefsNear(fg, [1.3, 2.0], dims=(1, 2))
    assert labels == ["l0", "x0"] and dens[0] > dens[1] > 0.0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_new_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbp.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(nbp_overlap_rec),offsetof(nbp_overlap_rec,lab),offsetof(nbp_overlap_rec,lbb),sizeof(nbp_overlap_opts),'
                   'offsetof(nbp_overlap_opts,min_coeff),offsetof(nbp_overlap_opts,topk),offsetof(nbp_overlap_opts,pad),'
                   'NBP_OVERLAP_MAXK);return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.OverlapRec), abi.OverlapRec.lab.offset, abi.OverlapRec.lbb.offset, C.sizeof(abi.OverlapOpts),
            abi.OverlapOpts.min_coeff.offset, abi.OverlapOpts.topk.offset, abi.OverlapOpts.pad.offset, abi.OVERLAP_MAXK]
    assert got == want
    assert (abi.OVERLAP_REACH, abi.OVERLAP_MIN_COEFF, abi.OVERLAP_TOPK) == (6.0, 1e-3, 8)
    hdr = open(os.path.join(ROOT, "include", "nbp.h")).read()
    for name, val in (("NBP_OVERLAP_REACH", "6.0"), ("NBP_OVERLAP_MIN_COEFF", "1e-3"), ("NBP_OVERLAP_TOPK", "8")):
        assert f"#define {name} {val}\n" in hdr
    for name in ("nbp_run_overlap", "nbp_kde_overlap", "nbp_run_overlap_search"):
        assert name in abi.EXPORTS
