"""-m gpu: factor likelihoods on the device (nbp_run_factor_likelihood / nbp_factor_likelihood, csrc/nbp_likelihood.h) through the C
ABI, the mirror and a solve session, held to the numpy restatement of tests/likelihood_cases.py.  The tolerance is worked out per
case on the host (likelihood_cases.restate): 16 max(|float64 - long double| of the restatement, 4 ulp(max(1, |l|)))."""
import copy
import ctypes as C

import numpy as np
import pytest

import likelihood_cases as lc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
lik = iif.likelihood

GROUPS = {g: [n for n in lc.CASES if n.startswith(g)] for g in ("prior", "linrel", "circ", "se2", "dist")}


def _load(be, names, counts, seed, first=0):
    """case i of `names` with the counts (n_a, n_b) -> its roles in slots first + 2 i and first + 2 i + 1; returns the descriptors
    and the host points [(A, B)]"""
    rng = np.random.default_rng(seed)
    slots, mans, bels, descs, pts = [], [], [], [], []
    for i, (name, (na, nb)) in enumerate(zip(names, counts)):
        A, B = lc.clouds(name, na, nb, rng)
        A, B, m = lc.points(name, A), lc.points(name, B), lc.CASES[name][1]
        sa, sb = first + 2 * i, first + 2 * i + 1
        slots.append(sa)
        mans.append(m)
        bw = np.ones(abi.MANIFOLD_DIM[m])  # (never read by the query; a belief of fewer than N points must bring one)
        bels.append((A, bw, None))
        if B is not None:
            slots.append(sb)
            mans.append(m)
            bels.append((B, bw, None))
        descs.append(lc.desc(name, sa, -1 if B is None else sb))
        pts.append((A, B))
    be.beliefs_write(slots, mans, bels)
    return descs, pts


def _check(be, names, descs, pts, what):
    ll, cl = be.run_factor_likelihood(descs)
    worst = 0.0
    for i, name in enumerate(names):
        worst = max(worst, lc.hold(ll[i], cl[i], lc.restate(descs[i], *pts[i]), f"{what} {name}"))
    print(f"{what}: largest error / tolerance {worst:.3f}")
    return ll, cl


# ---- 1. every kind x family x manifold at full count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("N", [8, 65, 200, 512])
def test_every_kind_family_and_manifold_at_full_count(hip_backend, N, group):
    names = GROUPS[group]
    be = hip_backend(N, 2 * len(names))
    try:
        descs, pts = _load(be, names, [(N, N)] * len(names), 500 + N)
        _check(be, names, descs, pts, f"N={N}")
    finally:
        be.close()


# ---- 2. counts below the context size and unequal in the two roles -------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(1, 150), (63, 2), (150, 1), (64, 65)])
def test_counts_below_the_context_size(hip_backend, counts):
    names = ["prior_se2_full", "linrel_e1_mix4", "linrel_e3_coords13", "circ_mix2", "se2_full", "se2_heading", "dist_e2_rayleigh", "dist_e3_normal"]
    be = hip_backend(200, 2 * len(names))
    try:
        descs, pts = _load(be, names, [counts] * len(names), 600 + counts[0])
        _check(be, names, descs, pts, f"counts {counts}")
    finally:
        be.close()


# ---- 3. many items in one launch ---------------------------------------------------------------------------------------------------------
def test_300_mixed_items_in_one_launch(hip_backend):
    names = ["linrel_e2_full", "se2_mix4", "prior_e3_full", "circ_uniform", "dist_e2_normal", "linrel_e1_mix4"]
    be = hip_backend(100, 2 * len(names))
    try:
        base, pts = _load(be, names, [(100, 70)] * len(names), 700)
        # 300 items (more than the chip has compute units); item 0 is repeated as the last one
        order = [(7 * k) % len(names) for k in range(1, 299)]
        descs = [base[0]] + [base[i] for i in order] + [base[0]]
        ll, cl = be.run_factor_likelihood(descs)
        assert len(ll) == 300 and ll[0].tobytes() == ll[-1].tobytes() and cl[0].tobytes() == cl[-1].tobytes()
        ll2, cl2 = be.run_factor_likelihood(descs)
        assert ll.tobytes() == ll2.tobytes() and cl.tobytes() == cl2.tobytes()
        single = [be.run_factor_likelihood([d]) for d in base]
        refs = [lc.restate(d, *p) for d, p in zip(base, pts)]
        for k, i in enumerate([0] + order + [0]):
            assert ll[k].tobytes() == single[i][0][0].tobytes() and cl[k].tobytes() == single[i][1][0].tobytes(), (k, i)
        for i, name in enumerate(names):
            lc.hold(single[i][0][0], single[i][1][0], refs[i], f"batch {name}")
    finally:
        be.close()


# ---- 4. underflow and support --------------------------------------------------------------------------------------------------------------
def test_underflow_and_support(hip_backend):
    be = hip_backend(64, 4)
    try:
        rng = np.random.default_rng(9)
        sigma = 0.2
        d = lik.likelihood_desc(abi.F_LINREL, abi.EUCLID1, [(1.0, [0.0], [[sigma]])], 0, 0, 1)
        for sigmas in (1e3, 1e4):
            A, B = rng.normal(0.0, 0.1, (50, 1)), rng.normal(sigmas * sigma, 0.1, (60, 1))
            be.beliefs_write([0, 1], [abi.EUCLID1] * 2, [(A, [1.0], None), (B, [1.0], None)])
            ll, cl = be.run_factor_likelihood([d])
            ll80, _ = lik.factor_likelihood_numpy(d, A, B, dtype=np.longdouble)
            print(f"{sigmas:g} sigma apart: device {ll[0]!r}, long double {ll80!r}")
            assert np.isfinite(ll[0]) and abs(float(ll[0] - ll80)) <= 1e-9 * abs(float(ll80))
            lc.hold(ll[0], cl[0], lc.restate(d, A, B), f"{sigmas:g} sigma")
        A = np.array([[0.0], [0.5]])
        be.belief_write(0, abi.EUCLID1, A, [1.0])
        for name, Bout, Bone in (("linrel_e1_uniform", [[5.0], [6.0]], [[5.0], [2.25]]), ("linrel_e1_rayleigh", [[-5.0], [-6.0]], [[-5.0], [0.25]])):
            d = lc.desc(name, 0, 1)
            be.belief_write(1, abi.EUCLID1, np.array(Bout), [1.0])
            ll, cl = be.run_factor_likelihood([d])
            assert ll[0] == -np.inf and cl[0, 0] == -np.inf and np.all(np.isnan(cl[0, 1:]))
            be.belief_write(1, abi.EUCLID1, np.array(Bone), [1.0])
            ll, cl = be.run_factor_likelihood([d])
            assert np.isfinite(ll[0])
            lc.hold(ll[0], cl[0], lc.restate(d, A, np.array(Bone)), f"{name} one pair inside")
        # a mixture with one component out of the support: its comp_loglik is -inf, the others finite
        d = lik.likelihood_desc(abi.F_PRIOR, abi.EUCLID1, [(0.5, [2.0], [[0.3]], lc.G), (0.5, [-1.0], [[2.0]], lc.U)], 0, 0, -1)
        X = rng.normal(2.05, 0.1, (64, 1))
        be.belief_write(0, abi.EUCLID1, X, [1.0])
        ll, cl = be.run_factor_likelihood([d])
        assert cl[0, 1] == -np.inf and np.isfinite(cl[0, 0])
        lc.hold(ll[0], cl[0], lc.restate(d, X, None), "prior mixture, uniform outside")
        # a belief without points (the host-buffer form: a slot always holds at least one): NaN, nothing launched
        ll0, cl0 = be.factor_likelihood(lc.desc("linrel_e1_normal"), np.zeros((0, 1)), X)
        assert np.isnan(ll0) and np.all(np.isnan(cl0))
    finally:
        be.close()


def test_host_buffer_form_equals_the_resident_form(hip_backend):
    be = hip_backend(100, 6)
    try:
        names = ["se2_full", "prior_e2_mix2", "dist_e3_normal"]
        descs, pts = _load(be, names, [(100, 80)] * 3, 800)
        ll, cl = be.run_factor_likelihood(descs)
        for i, name in enumerate(names):
            l1, c1 = be.factor_likelihood(lc.desc(name, 5, 5), *pts[i])  # (its own slots are not read)
            assert np.float64(l1).tobytes() == ll[i].tobytes() and c1.tobytes() == cl[i].tobytes(), name
    finally:
        be.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp = C.POINTER(C.c_double)
    try:
        rng = np.random.default_rng(61)
        for s in range(4):
            be.belief_write(s, abi.EUCLID1, rng.normal(0, 1, (64, 1)))
        good = lc.desc("linrel_e1_normal", 0, 1)
        out, comp = np.full(1, 7.0), np.full(abi.MAXC, 7.0)

        def call(d, n=1, o=out, c=comp, descs=True, context=ctx):
            arr = (abi.LikelihoodDesc * 1)(d)
            rc = lib.nbp_run_factor_likelihood(context, arr if descs else None, n, o.ctypes.data_as(dp) if o is not None else None,
                                               c.ctypes.data_as(dp) if c is not None else None)
            assert out[0] == 7.0 and np.all(comp == 7.0) or rc == 0, "a refused call leaves the outputs untouched"
            return rc

        def edit(name="linrel_e1_normal", sa=0, sb=1, **kw):
            d = lc.desc(name, sa, sb)
            for k, v in kw.items():
                if k.startswith("comp"):
                    d.comp[int(k[4])][int(k[6:])] = v
                else:
                    setattr(d, k, v)
            return d
        assert call(good, descs=False) == -1 and call(good, o=None) == -1 and call(good, context=None) == -1
        assert call(good, n=0) == 0 and lib.nbp_run_factor_likelihood(ctx, None, 0, None, None) == 0 and out[0] == 7.0
        ARG, RANGE = -1, -4
        refused = [
            (edit(kind=abi.F_MSGPRIOR), ARG), (edit(kind=abi.F_PASSTHROUGH), ARG), (edit(kind=0), ARG), (edit(kind=9), ARG),
            (edit(comp0_12=float(abi.DIST_TABLE)), ARG), (edit(comp0_12=5.0), ARG),
            (edit("linrel_e2_full", comp0_5=0.25), ARG),                                # a non-zero above the diagonal
            (edit(comp0_4=0.0), ARG), (edit(comp0_4=-1.0), ARG), (edit(comp0_4=np.inf), ARG), (edit(comp0_4=np.nan), ARG),
            (edit("linrel_e2_full", comp0_8=0.0), ARG),
            (edit("linrel_e1_uniform", comp0_4=0.0), ARG), (edit("linrel_e1_uniform", comp0_4=np.inf), ARG),
            (edit("linrel_e1_rayleigh", comp0_4=-2.0), ARG), (edit("linrel_e1_rayleigh", comp0_4=np.nan), ARG),
            (edit(ncomp=0), ARG), (edit(ncomp=5), ARG),
            (edit(comp0_0=-1.0), ARG), (edit(comp0_0=0.0), ARG),
            (edit(kind=abi.F_CIRCULAR), ARG), (edit(kind=abi.F_SE2), ARG), (edit(manifold=abi.CIRCULAR), ARG), (edit(manifold=abi.SE2), ARG),
            (edit(kind=abi.F_EUCLIDDIST, manifold=abi.SE2), ARG), (edit(manifold=0), ARG), (edit(manifold=6), ARG),
            (edit("prior_e1_normal", sb=1), ARG),                                       # a prior is unary
            (edit(kind=abi.F_EUCLIDDIST, partial_mask=1), ARG), (edit("linrel_e3_full", partial_mask=7), ARG),
            (edit(partial_mask=2), RANGE), (edit(partial_mask=-1), RANGE), (edit("prior_e2_full", sb=-1, partial_mask=4), RANGE),
            (edit(sa=-1), RANGE), (edit(sa=4), RANGE), (edit(sb=4), RANGE), (edit(sb=-2), RANGE), (edit(sb=-1), RANGE),
        ]
        for i, (d, status) in enumerate(refused):
            assert call(d) == status, (i, lib.nbp_last_error())
        two = (abi.LikelihoodDesc * 2)(good, edit(sa=9))
        assert lib.nbp_run_factor_likelihood(ctx, two, 2, np.zeros(2).ctypes.data_as(dp), None) == RANGE and b"item 1" in lib.nbp_last_error()
        with pytest.raises(iif.NbpError, match="-4"):
            be.run_factor_likelihood([edit(sb=4)])
        # the host-buffer form
        a = np.ascontiguousarray(rng.normal(0, 1, (10, 1)))
        ap, o1 = a.ctypes.data_as(dp), C.c_double(7.0)
        assert lib.nbp_factor_likelihood(ctx, None, ap, 10, ap, 10, C.byref(o1), None) == -1
        assert lib.nbp_factor_likelihood(ctx, C.byref(good), None, 10, ap, 10, C.byref(o1), None) == -1
        assert lib.nbp_factor_likelihood(ctx, C.byref(good), ap, 10, None, 10, C.byref(o1), None) == -1
        assert lib.nbp_factor_likelihood(ctx, C.byref(good), ap, 10, ap, 10, None, None) == -1
        assert lib.nbp_factor_likelihood(ctx, C.byref(edit(comp0_4=0.0)), ap, 10, ap, 10, C.byref(o1), None) == -1 and o1.value == 7.0
        assert lib.nbp_factor_likelihood(ctx, C.byref(good), ap, 10, ap, 10, C.byref(o1), None) == 0 and np.isfinite(o1.value)
        assert lib.nbp_factor_likelihood(ctx, C.byref(lc.desc("prior_e1_normal")), ap, 10, None, 0, C.byref(o1), None) == 0
        # a valid call still works on the same context (the host-buffer calls above left their points in slots 0 and 1)
        assert call(good, c=None) == 0 and np.isfinite(out[0]) and np.all(comp == 7.0)
        lc.hold(*[r[0] for r in be.run_factor_likelihood([good])], lc.restate(good, a, a), "after the refusals")
    finally:
        be.close()


# ---- 6. the mirror -------------------------------------------------------------------------------------------------------------------------
def _hold_to_numpy(fg, got, what):
    """every factor's device answer against the restatement on the host copies of the beliefs"""
    for label, r in got.items():
        plan = lik.factor_items(fg, label)
        for k, (d, (a, b)) in enumerate(zip(plan.descs, plan.roles)):
            ref = lc.restate(d, fg.getVal(a), None if b is None else fg.getVal(b))
            ll = r.hypo_loglik[k] if plan.hypotheses else r.loglik
            cl = np.full(abi.MAXC, np.nan)
            cl[:d.ncomp] = r.comp_loglik[k] if plan.hypotheses else r.comp_loglik
            lc.hold(ll, cl, ref, f"{what} {label}[{k}]")
        host = iif.factorLikelihood(fg, label)
        assert host.hypotheses == r.hypotheses and host.hypo_prior.tobytes() == r.hypo_prior.tobytes()
        if r.hypotheses and np.isfinite(host.hypo_loglik).all():
            assert np.abs(host.hypo_weights - r.hypo_weights).max() < 1e-9


def test_mirror_on_a_hand_set_graph(hip_backend):
    fg = lc.doors_graph()
    bad = lc.outlier_chain(fg)
    iif.addFactor(fg, ["x"], iif.Mixture(iif.Prior, [iif.Normal(2.0, 0.3), iif.Uniform(-1.0, 1.0)], [0.5, 0.5]), label="xmix")
    every = iif.factorLikelihoodAll(fg, backend=hip_backend)
    assert list(every) == ["door", "p0f1", "p0p1f1", "p1p2f1", "p2p3f1", "p3p4f1", "p4p5f1", "xmix"] and every.skipped == []
    _hold_to_numpy(fg, every, "hand-set")
    assert every["door"].hypo_weights[1] > 1 - 1e-12
    ranked = sorted((l for l in every if l.startswith("p")), key=lambda l: every[l].loglik)
    assert ranked[0] == bad and every[bad].loglik < -400 and every[ranked[1]].loglik > 0  # (the bounds: test_factor_likelihood.py)
    one = iif.factorLikelihood(fg, "door", backend=hip_backend)
    assert one.hypo_loglik.tobytes() == every["door"].hypo_loglik.tobytes() and np.float64(one.loglik).tobytes() == np.float64(every["door"].loglik).tobytes()
    fg.factors["msg"] = iif.factorgraph.DFGFactor("msg", ["x"], iif.factorgraph.MsgPrior(3))
    assert iif.factorLikelihoodAll(fg, backend=hip_backend).skipped == ["msg"]
    with pytest.raises(ValueError, match="factor msg:"):
        iif.factorLikelihood(fg, "msg", backend=hip_backend)


def test_mirror_on_the_posteriors_of_a_device_solve(hip_backend):
    fg = iif.generateChainEuclid(10, vardims=2, priorEvery=5, N=64)
    iif.solveTree(fg, backend=hip_backend, seed=3)
    got = iif.factorLikelihoodAll(fg, backend=hip_backend)
    assert len(got) == len(fg.lsf()) and got.skipped == []
    _hold_to_numpy(fg, got, "chain")
    assert all(np.isfinite(r.loglik) for r in got.values())


# ---- 7. the session ------------------------------------------------------------------------------------------------------------------------
def test_session_reads_the_resident_beliefs_where_they_lie(hip_backend):
    """the circular-doors graph (multihypo sightings of doors): after a solve, every factor's likelihood from ONE launch on the resident
    beliefs; `stats` does not move; after invalidate(v) exactly that belief goes up"""
    fg = iif.generateCircularDoors(nposes=10, N=64, sightEvery=5)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=71)
        before = copy.deepcopy(ses.stats)
        got = ses.factorLikelihoods()
        assert ses.stats == before
        host = iif.factorLikelihoodAll(fg, backend=hip_backend)
        assert list(got) == list(host) and got.skipped == host.skipped and len(got) > 10
        assert any(r.hypotheses for r in got.values()), "the graph has multihypo sightings"
        for label in got:
            # the same beliefs on the same device: the session's slots hold what the host copy was read back from
            assert np.float64(got[label].loglik).tobytes() == np.float64(host[label].loglik).tobytes(), label
            assert got[label].comp_loglik.tobytes() == host[label].comp_loglik.tobytes() and got[label].hypo_weights.tobytes() == host[label].hypo_weights.tobytes()
        _hold_to_numpy(fg, got, "session")
        some = list(got)[:3]
        assert list(ses.factorLikelihoods(some)) == some and ses.stats == before
        ses.invalidate("x3")
        again = ses.factorLikelihoods()
        assert ses.stats["uploads"] == before["uploads"] + 1 and ses.stats["readbacks"] == before["readbacks"]
        assert all(np.float64(again[l].loglik).tobytes() == np.float64(got[l].loglik).tobytes() for l in got)
        assert ses.factorLikelihoods().keys() == got.keys() and ses.stats["uploads"] == before["uploads"] + 1
