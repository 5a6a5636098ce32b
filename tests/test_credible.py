"""CPU: the definition of the credible regions (incrementalinference.jl_amd/credible.py) as credible_numpy restates it --
hand-written values, the special cases, the ABI mirror, the calibration of the definition, and the conditions under which
tests/test_gpu_credible.py compares the device's counts with numpy's (tests/credible_cases.py derives every bound)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import credible_cases as cc
import ppe_cases as pc
from parity_utils import abi, iif

cr = iif.credible
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


# ---- hand-written values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", cc.MANIFOLDS)
def test_two_points_have_one_density(man):
    rng = np.random.default_rng(3)
    X = pc.cloud("gaussian", man, 2, rng)
    r = cr.credible_numpy(man, pc.to_points(man, X), pc.hand_bandwidth(man), cc.full_mask(man), (0.5, 1.0), ())
    assert r.logdens[0].tobytes() == r.logdens[1].tobytes() and np.isfinite(r.logdens).all()
    assert r.order.tolist() == [0, 1] and r.n_inside.tolist() == [2, 2]
    assert r.log_levels[0] == r.log_levels[1] == r.logdens[0] == r.log_min == r.log_max


def test_three_collinear_points_by_hand():
    """x = 0, 1, 3 with h = 1: l_0 = log((e^-1/2 + e^-9/2) / 2) - log sqrt(2 pi), l_1 = log((e^-1/2 + e^-2) / 2) - ..., l_2 =
    log((e^-9/2 + e^-2) / 2) - ...; the middle point is the densest, the far one the thinnest"""
    r = cr.credible_numpy(abi.EUCLID1, np.array([[0.0], [1.0], [3.0]]), [1.0], 1, (1.0 / 3, 2.0 / 3, 1.0), (), queries=[[1.0]])
    want = np.array([math.log((math.exp(-0.5) + math.exp(-4.5)) / 2), math.log((math.exp(-0.5) + math.exp(-2.0)) / 2),
                     math.log((math.exp(-4.5) + math.exp(-2.0)) / 2)]) - LOG_SQRT_2PI
    assert np.abs(r.logdens - want).max() <= 4e-16 * 4, (r.logdens, want)
    assert r.order.tolist() == [2, 0, 1]
    assert r.log_levels.tolist() == [r.logdens[1], r.logdens[0], r.logdens[2]] and r.n_inside.tolist() == [1, 2, 3]
    # the query at the middle point: all three kernels, normalised by 3 -- denser than every leave-one-out value
    lq = math.log((math.exp(-0.5) + 1.0 + math.exp(-2.0)) / 3) - LOG_SQRT_2PI
    assert abs(r.q_logdens[0] - lq) <= 1e-15 and r.q_n_above.tolist() == [0] and r.q_mass.tolist() == [0.0]


@pytest.mark.parametrize("c", [1, 2, 5, 200])
def test_quantiles_of_a_ramp_are_exact(c):
    probs = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0, 1.0 / 3)
    perm = np.random.default_rng(c).permutation(c)
    r = cr.credible_numpy(abi.EUCLID1, np.arange(c, dtype=np.float64)[perm, None], [1.0], 1, (), probs)
    assert r.quantiles[0].tolist() == [float(c - 1) * p for p in probs]


@pytest.mark.parametrize("c", [2, 3, 64, 200, 511])
def test_quantiles_agree_with_numpy_within_two_ulp(c):
    """np.quantile forms the same type-7 value by another lerp (b - (b - a) (1 - g) from g = 1/2 on).  Both forms round a
    difference and a product of the size of |b - a| and a sum of the size of the larger of the two order statistics a, b: the ulp
    meant is that of max(|a|, |b|) -- where a and b differ in sign the quantile itself can be arbitrarily small beside them."""
    rng = np.random.default_rng(100 + c)
    probs = np.concatenate([[0.0, 1.0, 0.5], rng.uniform(size=5)])
    X = rng.normal(2.0, 3.0, (c, 3))
    r = cr.credible_numpy(abi.EUCLID3, X, [1.0, 1.0, 1.0], 1, (), probs)
    want = np.quantile(X, probs, axis=0, method="linear").T
    S = np.sort(X, axis=0)
    lo = np.floor((c - 1) * probs).astype(int)
    big = np.maximum(np.abs(S[lo]), np.abs(S[np.minimum(lo + 1, c - 1)])).T
    assert np.all(np.abs(r.quantiles - want) <= 2 * np.spacing(big)), (np.abs(r.quantiles - want) / np.spacing(big)).max()


def test_level_rank_table():
    """k = ceil(a (double)c), in double as written: 0.95 * 200 rounds to 190.0 and 0.9 * 150 to 135.0, 0.95 * 150 to 142.5"""
    table = {1: (1, 1, 1, 1, 1), 2: (1, 2, 2, 2, 1), 63: (32, 57, 60, 63, 1), 150: (75, 135, 143, 150, 1), 200: (100, 180, 190, 200, 1),
             512: (256, 461, 487, 512, 1)}
    for c, want in table.items():
        assert tuple(cr.level_rank(a, c) for a in (0.5, 0.9, 0.95, 1.0, 1e-9)) == want, c
    rng = np.random.default_rng(5)
    for c in table:
        X = rng.normal(size=(c, 1))
        r = cr.credible_numpy(abi.EUCLID1, X, [0.5], 1, (0.5, 0.9, 0.95, 1.0, 1e-9), ())
        if c == 1:
            assert np.isnan(r.log_levels).all()
            continue
        ls = np.sort(r.logdens)
        assert r.log_levels.tolist() == [ls[c - k] for k in table[c]]
        assert r.n_inside.tolist() == (list(table[c]) if c > 2 else [2] * 5)  # (no ties in a random cloud; two points always tie)


@pytest.mark.parametrize("man", [abi.CIRCULAR, abi.SE2])
def test_quantiles_straddle_pi(man):
    rng = np.random.default_rng(8)
    X = pc.cloud("across_pi", man, 200, rng)
    d = pc.circular_coords(man)[0]
    assert (X[:, d] > 2).any() and (X[:, d] < -2).any()  # the cloud lies on both sides of +-pi
    probs = (0.025, 0.25, 0.5, 0.75, 0.975)
    r = cr.credible_numpy(man, pc.to_points(man, X), pc.hand_bandwidth(man), cc.full_mask(man), (), probs)
    q = r.quantiles[d]
    off = pc.wrap(q - np.pi)  # about the cloud's centre the quantiles ascend; as plain numbers they jump from +pi to -pi
    assert np.all(np.diff(off) > 0) and abs(off[2]) < 0.1 and off[0] < -0.4 and off[4] > 0.4, off
    assert q[0] > 2 and q[4] < -2, q
    assert np.all((q >= -np.pi) & (q < np.pi))
    want = np.quantile(pc.wrap(X[:, d] - np.pi), probs)  # the cloud unrolled about its centre
    assert np.abs(off - want).max() < 1e-12


@pytest.mark.parametrize("man", cc.MANIFOLDS)
def test_identical_points_tie(man):
    rng = np.random.default_rng(9)
    c = 37
    X = pc.cloud("identical", man, c, rng)
    r = cr.credible_numpy(man, pc.to_points(man, X), pc.hand_bandwidth(man), cc.full_mask(man), cc.MASS, cc.PROBS)
    assert np.all(r.logdens == r.logdens[0]) and np.isfinite(r.logdens[0])
    assert r.order.tolist() == list(range(c)) and np.all(r.n_inside == c)
    if man != abi.SE2:
        assert np.all(r.quantiles == X[0][:, None])


@pytest.mark.parametrize("man", [abi.EUCLID1, abi.EUCLID2, abi.EUCLID3])
def test_own_point_and_far_query(man):
    D = abi.MANIFOLD_DIM[man]
    rng = np.random.default_rng(10 + D)
    X, h = pc.cloud("gaussian", man, 200, rng), pc.hand_bandwidth(man)
    Q = cc.queries_for(man, X, h, rng, 2)[:, :D]
    r = cr.credible_numpy(man, X, h, cc.full_mask(man), (0.9,), (), Q)
    # the own point: c p(x_0) = (c - 1) p_loo(x_0) + K(0)
    k0 = -D * LOG_SQRT_2PI - float(np.log(h).sum())
    want = math.log(199 * math.exp(r.logdens[0]) + math.exp(k0)) - math.log(200)
    assert abs(r.q_logdens[0] - want) <= 1e-12 * (1 + abs(want))
    # 1e3 bandwidths away: every term underflows, the logarithm does not
    assert np.isfinite(r.q_logdens[1]) and r.q_logdens[1] < -4e5 * D
    assert r.q_n_above[1] == 200 and r.q_mass[1] == 1.0 and r.q_mass[1].tobytes() == np.float64(1.0).tobytes()
    assert 0 <= r.q_n_above[0] < 200 and r.q_mass[0] == r.q_n_above[0] / 200


def test_one_point_has_no_level():
    r = cr.credible_numpy(abi.EUCLID2, [[1.5, -2.0]], [0.3, 0.4], 3, (0.5, 0.95), (0.0, 0.5, 1.0), [[1.5, -2.0]])
    assert np.isnan(r.logdens).all() and np.isnan(r.log_levels).all() and r.order.tolist() == [0] and r.count == 1
    assert np.isnan(r.log_min) and np.isnan(r.log_max) and r.n_inside.tolist() == [0, 0]
    assert r.quantiles.tolist() == [[1.5] * 3, [-2.0] * 3] and r.mean.tolist() == [1.5, -2.0]
    assert np.isnan(r.q_mass).all() and r.q_n_above.tolist() == [-1]
    assert abs(r.q_logdens[0] - (-2 * LOG_SQRT_2PI - math.log(0.3 * 0.4))) <= 1e-15


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, math.inf])
def test_bad_bandwidth_in_the_mask(bad):
    rng = np.random.default_rng(12)
    X = rng.normal(size=(50, 3))
    good = cr.credible_numpy(abi.EUCLID3, X, [0.3, 0.4, 0.2], 3, (0.5,), (0.5,), X[:2])
    r = cr.credible_numpy(abi.EUCLID3, X, [0.3, bad, 0.2], 3, (0.5,), (0.5,), X[:2])
    assert np.isnan(r.logdens).all() and np.isnan(r.log_levels).all() and np.all(r.order == -1)
    assert np.isnan(r.q_logdens).all() and np.isnan(r.q_mass).all() and np.all(r.q_n_above == -1)
    assert r.quantiles.tobytes() == good.quantiles.tobytes() and r.mean.tobytes() == good.mean.tobytes()
    # outside the mask the entry is not looked at
    r = cr.credible_numpy(abi.EUCLID3, X, [0.3, 0.4, bad], 3, (0.5,), (0.5,), X[:2])
    assert r.logdens.tobytes() == good.logdens.tobytes() and r.q_mass.tobytes() == good.q_mass.tobytes()


def test_masks_select_coordinates():
    """the density on K of a D-dimensional belief is the density of the belief cut down to K"""
    rng = np.random.default_rng(13)
    X, h = pc.cloud("gaussian", abi.SE2, 60, rng), pc.hand_bandwidth(abi.SE2)
    r = cr.credible_numpy(abi.SE2, pc.to_points(abi.SE2, X), h, 3, (0.9,), (), X[:3])
    e2 = cr.credible_numpy(abi.EUCLID2, X[:, :2], h[:2], 3, (0.9,), (), X[:3, :2])
    assert r.logdens.tobytes() == e2.logdens.tobytes() and r.q_logdens.tobytes() == e2.q_logdens.tobytes()
    with pytest.raises(ValueError):
        cr.credible_numpy(abi.EUCLID2, X[:, :2], h[:2], 4)
    with pytest.raises(ValueError):
        cr.credible_numpy(abi.EUCLID2, X[:, :2], h[:2], 0)


def test_coverage_and_inside():
    assert cr.coverage([0.1, 0.6, 0.92, 0.99, math.nan]).tolist() == [0.25, 0.5, 0.75]
    assert cr.coverage({"a": cr.Credibility(0.5, -1.0, 3), "b": cr.Credibility(np.array([0.2, 0.97]), None, None)}, at=(0.5, 0.9)).tolist() == [2 / 3, 2 / 3]
    reg = cr.CredibleRegion(np.array([0.5, 0.9]), np.array([-1.0, -2.0]), np.exp([-1.0, -2.0]), np.array([2, 3]), np.zeros(0), np.zeros((1, 0)),
                            np.zeros(1), 4, np.array([-0.5, -1.0, -1.5, -3.0]), np.array([3, 2, 1, 0]))
    assert reg.inside(0.9).tolist() == [True, True, True, False] and reg.inside(0.5).tolist() == [True, True, False, False]
    with pytest.raises(KeyError):
        reg.inside(0.7)
    assert iif.credibleRegion is cr.credibleRegion and iif.credibility is cr.credibility and iif.coverage is cr.coverage
    q, single = cr.query_points(abi.SE2, (1, 2), [1.0, 2.0])
    assert q.tolist() == [[1.0, 2.0, 0.0]] and single
    q, single = cr.query_points(abi.SE2, (3,), [[0.5], [0.25]])
    assert q.tolist() == [[0.0, 0.0, 0.5], [0.0, 0.0, 0.25]] and not single
    with pytest.raises(ValueError):
        cr.query_points(abi.EUCLID2, None, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        cr.query_points(abi.EUCLID2, None, [1.0, math.inf])
    for bad in (dict(mass=(0.0,)), dict(mass=(1.5,)), dict(probs=(-0.1,)), dict(probs=(math.nan,)), dict(mass=(0.5,) * 9)):
        with pytest.raises(ValueError):
            cr._options(bad.get("mass", (0.5,)), bad.get("probs", (0.5,)))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_names_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbp.h"\nint main(){printf("' + "%zu " * 14 + '%d\\n",'
                   'sizeof(nbp_credible_opts),offsetof(nbp_credible_opts,n_prob),offsetof(nbp_credible_opts,mass),offsetof(nbp_credible_opts,prob),'
                   'sizeof(nbp_credible_rec),offsetof(nbp_credible_rec,quant),offsetof(nbp_credible_rec,mean),offsetof(nbp_credible_rec,log_min),'
                   'offsetof(nbp_credible_rec,log_max),offsetof(nbp_credible_rec,n_inside),offsetof(nbp_credible_rec,count),'
                   'sizeof(nbp_credibility_rec),offsetof(nbp_credibility_rec,mass),offsetof(nbp_credibility_rec,n_above),NBP_CRED_MAX);return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    O, R, Q = abi.CredibleOpts, abi.CredibleRec, abi.CredibilityRec
    want = [C.sizeof(O), O.n_prob.offset, O.mass.offset, O.prob.offset, C.sizeof(R), R.quant.offset, R.mean.offset, R.log_min.offset,
            R.log_max.offset, R.n_inside.offset, R.count.offset, C.sizeof(Q), Q.mass.offset, Q.n_above.offset, abi.CRED_MAX]
    assert got == want and got[0] == 136 and got[4] == 336 and got[11] == 24 and got[-1] == 8
    rec, qrec = iif.HipBackend.CRED_REC, iif.HipBackend.CREDIBILITY_REC
    assert rec.itemsize == C.sizeof(R) and qrec.itemsize == C.sizeof(Q)
    for name in ("log_level", "quant", "mean", "log_min", "log_max", "n_inside", "count", "pad"):
        assert rec.fields[name][1] == getattr(R, name).offset, name
    for name in ("logdens", "mass", "n_above", "pad"):
        assert qrec.fields[name][1] == getattr(Q, name).offset, name
    hdr = open(os.path.join(ROOT, "include", "nbp.h")).read()
    assert "#define NBP_CRED_MAX 8\n" in hdr
    for name in ("nbp_run_credible", "nbp_kde_credible"):
        assert name in abi.EXPORTS and name + "(" in hdr
    for method in ("run_credible", "kde_credible"):
        assert callable(getattr(iif.HipBackend, method))
    for method in ("credibleRegions", "credibility"):
        assert callable(getattr(iif.SolveSession, method))
    assert callable(iif.Belief.credible) and callable(iif.Belief.credibility)


# ---- the conditions of the device comparison ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.SCENARIOS)
def test_seeds_meet_the_conditions_of_the_device_comparison(name):
    N, items, masks, nq, seed = cc.scenario(name)
    worst = np.inf
    for (m, kind, c), k, (X, h, Q) in zip(items, masks, cc.beliefs(items, nq, seed)):
        D = abi.MANIFOLD_DIM[m]
        ref = cr.credible_numpy(m, pc.to_points(m, X), h, k, cc.MASS, cc.PROBS, Q[:, :D])
        cond = cc.conditions(m, k, X, ref.mean, ref, Q[:, :D], cc.MASS, ties=cc.exact_ties(kind, c))
        assert cond > 1.0, (name, m, kind, c, k, cond)
        worst = min(worst, cond)
    print(f"{name}: {len(items)} beliefs, the tightest condition holds {worst:.3g} times over")


# ---- calibration of the definition -------------------------------------------------------------------------------------------------
def test_leave_one_out_regions_are_calibrated_and_self_term_regions_are_not():
    loo, own = cc.calibration(cc.CAL_T, cc.CAL_SEED)
    for a in (0.5, 0.95):
        bound = cc.calibration_bound(a, cc.CAL_T)
        print(f"nominal {a}: leave-one-out {loo[a]:.4f}, self term in {own[a]:.4f}, bound {bound:.4f}")
    for a in (0.5, 0.95):
        assert abs(loo[a] - a) <= cc.calibration_bound(a, cc.CAL_T), (a, loo[a])
    assert abs(own[0.95] - 0.95) > cc.calibration_bound(0.95, cc.CAL_T), own
    assert own[0.95] < 0.95 and own[0.5] < 0.5  # too small, not too large: the regions of the self-term variant under-cover
