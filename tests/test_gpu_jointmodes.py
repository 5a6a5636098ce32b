"""-m gpu: mode-by-mode factor likelihoods on the device (nbp_run_factor_mode_likelihood / nbp_factor_mode_likelihood,
csrc/nbp_likelihood.h) through the C ABI, the mirror and a solve session, held to the numpy restatement of tests/jointmodes_cases.py.
The tolerance is worked out per cell on the host (jointmodes_cases.restate): 16 max(|float64 - long double| of the restatement,
4 ulp(max(1, |T|)))."""
import copy
import ctypes as C

import numpy as np
import pytest

import jointmodes_cases as jc
import likelihood_cases as lc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
MAXK = abi.MAXK

GROUPS = {g: [n for n in lc.CASES if n.startswith(g)] for g in ("prior", "linrel", "circ", "se2", "dist")}
SHAPE_CASES = ["linrel_e2_full", "linrel_e1_mix4", "se2_full"]  # a relative Gaussian, a mixture, SE(2)


def _load(be, names, counts, seed):
    """case i of `names` with the counts (n_a, n_b) -> its roles in slots 2 i and 2 i + 1; returns the descriptors and the host
    points [(A, B)]"""
    rng = np.random.default_rng(seed)
    slots, mans, bels, descs, pts = [], [], [], [], []
    for i, (name, (na, nb)) in enumerate(zip(names, counts)):
        A, B = lc.clouds(name, na, nb, rng)
        A, B, m = lc.points(name, A), lc.points(name, B), lc.CASES[name][1]
        bw = np.ones(abi.MANIFOLD_DIM[m])
        slots.append(2 * i)
        mans.append(m)
        bels.append((A, bw, None))
        if B is not None:
            slots.append(2 * i + 1)
            mans.append(m)
            bels.append((B, bw, None))
        descs.append(lc.desc(name, 2 * i, -1 if B is None else 2 * i + 1))
        pts.append((A, B))
    be.beliefs_write(slots, mans, bels)
    return descs, pts


def _row(lab, N):
    """a label row of the launch: the labels, then garbage-free padding the kernel never reads"""
    r = np.full(N, -1, dtype=np.int32)
    r[:len(lab)] = lab
    return r


def _hold_items(be, items, what):
    """items: [(desc, (A, B), labels_a, labels_b)] in ONE launch, every table held to its restatement; the counts to np.bincount"""
    rows, ra, rb = [], [], []
    for d, (A, B), la, lb in items:
        ra.append(len(rows))
        rows.append(_row(la, be.N))
        if B is None:
            rb.append(-1)
        else:
            rb.append(len(rows))
            rows.append(_row(lb, be.N))
    tab, cnt = be.run_factor_mode_likelihood([it[0] for it in items], ra, rb, np.stack(rows))
    worst, terms = 0.0, {}
    for i, (d, (A, B), la, lb) in enumerate(items):
        if id(d) not in terms:
            terms[id(d)] = jc.pair_terms(d, A, B)
        ref = jc.restate(d, A, la, B, lb, terms[id(d)])
        assert np.array_equal(cnt[i], ref[1]), (what, i)
        assert np.array_equal(cnt[i, 0], np.bincount(la[la >= 0], minlength=MAXK))
        worst = max(worst, jc.hold(tab[i], ref, f"{what} item {i}"))
    print(f"{what}: largest error / tolerance {worst:.3f}")
    return tab, cnt


# ---- 1. every kind x family x manifold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_every_kind_family_and_manifold(hip_backend, group):
    names = GROUPS[group]
    be = hip_backend(200, 2 * len(names))
    try:
        descs, pts = _load(be, names, [(200, 150)] * len(names), 900)
        rng = np.random.default_rng(901)
        _hold_items(be, [(d, p, jc.labels(rng, 200, 2), jc.labels(rng, 150, 3)) for d, p in zip(descs, pts)], f"2x3 {group}")
    finally:
        be.close()


# ---- 2. the shapes where this kernel can go wrong -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 65, 200, 500])
def test_shapes(hip_backend, N):
    """part of a wave, one lane into the second wave, several waves; 1 x 1, 1 x 8, 8 x 1, 8 x 8 groups; a group whose members all sit in
    the last wave; an empty group in the middle; 30 % of the points labelled -1; n_b < N"""
    be = hip_backend(N, 4 * len(SHAPE_CASES))
    try:
        nb = max(N - 3, 1)
        full, pf = _load(be, SHAPE_CASES, [(N, N)] * 3, 910 + N)
        rng = np.random.default_rng(920 + N)
        items = []
        for d, p in zip(full, pf):
            for ka, kb in ((1, 1), (1, 8), (8, 1), (8, 8)):
                items.append((d, p, jc.labels(rng, N, ka), jc.labels(rng, N, kb)))
            items.append((d, p, jc.labels(rng, N, 3, last=2), jc.labels(rng, N, 3, last=1)))
            items.append((d, p, jc.labels(rng, N, 4, empty=1), jc.labels(rng, N, 4, empty=2)))
            items.append((d, p, jc.labels(rng, N, 2, minus=0.3), jc.labels(rng, N, 3, minus=0.3)))
        _hold_items(be, items, f"N={N}")
        # n_b < N: the label row's entries beyond the count are not members
        short, ps = _load(be, SHAPE_CASES, [(N, nb)] * 3, 930 + N)
        _hold_items(be, [(d, p, jc.labels(rng, N, 2), jc.labels(rng, nb, 3)) for d, p in zip(short, ps)], f"N={N} n_b={nb}")
    finally:
        be.close()


# ---- 3. one group: the factor-likelihood kernel's number bit for bit ------------------------------------------------------------------------
def test_one_group_equals_run_factor_likelihood_bit_for_bit(hip_backend):
    names = list(lc.CASES)
    be = hip_backend(200, 2 * len(names))
    try:
        descs, _ = _load(be, names, [(200, 150)] * len(names), 940)
        ll, _ = be.run_factor_likelihood(descs)
        n = len(names)
        zeros = np.zeros((1, 200), dtype=np.int32)
        t0, c0 = be.run_factor_mode_likelihood(descs, [0] * n, [-1 if lc.unary(x) else 0 for x in names], zeros)
        t1, c1 = be.run_factor_mode_likelihood(descs, [-1] * n, [-1] * n, np.zeros((0, 200), dtype=np.int32))
        for i, name in enumerate(names):
            assert np.array_equal(t0[i, 0, 0], ll[i]) and np.array_equal(t1[i, 0, 0], ll[i]), (name, t0[i, 0, 0], t1[i, 0, 0], ll[i])
            assert np.isnan(t0[i]).sum() == MAXK * MAXK - 1 and np.isnan(t1[i]).sum() == MAXK * MAXK - 1
            assert c0[i, 0, 0] == 200 and c0[i, 1, 0] == (1 if lc.unary(name) else 150) and np.array_equal(c0[i], c1[i])
    finally:
        be.close()


# ---- 4. many items in one launch ----------------------------------------------------------------------------------------------------------------
def test_300_mixed_items_in_one_launch(hip_backend):
    names = ["linrel_e2_full", "se2_mix4", "prior_e3_full", "circ_uniform", "dist_e2_normal", "linrel_e1_mix4"]
    be = hip_backend(100, 2 * len(names))
    try:
        base, pts = _load(be, names, [(100, 70)] * len(names), 950)
        rng = np.random.default_rng(951)
        # six label rows shared by all items, of 1, 2, 3, 5 and 8 groups, one with points left out
        rows = np.stack([_row(jc.labels(rng, 100, k, minus=m), 100) for k, m in ((1, 0), (2, 0), (3, 0.2), (5, 0), (8, 0), (2, 0))])
        pick = [(7 * k) % len(names) for k in range(300)]
        ra = [(3 * k) % 6 for k in range(300)]
        rb = [-1 if lc.unary(names[i]) else (5 * k + 1) % 6 for k, i in enumerate(pick)]
        tab, cnt = be.run_factor_mode_likelihood([base[i] for i in pick], ra, rb, rows)
        assert tab.shape == (300, MAXK, MAXK)
        tab2, cnt2 = be.run_factor_mode_likelihood([base[i] for i in pick], ra, rb, rows)
        assert tab.tobytes() == tab2.tobytes() and cnt.tobytes() == cnt2.tobytes()
        seen = {}
        for k, i in enumerate(pick):
            key = (i, ra[k], rb[k])
            if key not in seen:
                seen[key] = be.run_factor_mode_likelihood([base[i]], [ra[k]], [rb[k]], rows)
            t, c = seen[key]
            assert np.array_equal(tab[k], t[0], equal_nan=True) and tab[k].tobytes() == t[0].tobytes(), k
            assert np.array_equal(cnt[k], c[0])
            na, nb = 100, (1 if rb[k] < 0 else 70)
            la = rows[ra[k], :na]
            assert np.array_equal(cnt[k, 0], np.bincount(la[la >= 0], minlength=MAXK))
            lb = np.zeros(1, dtype=np.int32) if rb[k] < 0 else rows[rb[k], :nb]
            assert np.array_equal(cnt[k, 1], np.bincount(lb[lb >= 0], minlength=MAXK))
        for key in list(seen)[:12]:
            i, a, b = key
            jc.hold(seen[key][0][0], jc.restate(base[i], pts[i][0], rows[a, :100], pts[i][1], None if b < 0 else rows[b, :70]), f"batch {key}")
    finally:
        be.close()


def test_host_buffer_form_equals_the_resident_form(hip_backend):
    be = hip_backend(100, 6)
    try:
        names = ["se2_full", "prior_e2_mix2", "dist_e3_normal"]
        descs, pts = _load(be, names, [(100, 80)] * 3, 960)
        rng = np.random.default_rng(961)
        la, lb = jc.labels(rng, 100, 3, minus=0.1), jc.labels(rng, 80, 2)
        tab, cnt = be.run_factor_mode_likelihood(descs, [0] * 3, [1, -1, 1], np.stack([_row(la, 100), _row(lb, 100)]))
        for i, name in enumerate(names):
            t, c = be.factor_mode_likelihood(lc.desc(name, 5, 5), pts[i][0], la, pts[i][1], lb)  # (its own slots are not read)
            assert t.tobytes() == tab[i].tobytes() and np.array_equal(c, cnt[i]), name
        t, c = be.factor_mode_likelihood(lc.desc("se2_full"), pts[0][0], None, pts[0][1], None)
        ll, _ = be.factor_likelihood(lc.desc("se2_full"), *pts[0])
        assert np.array_equal(t[0, 0], ll) and c[0, 0] == 100 and c[1, 0] == 80
        # a belief without points: NaN, nothing launched
        t, c = be.factor_mode_likelihood(lc.desc("linrel_e1_normal"), np.zeros((0, 1)), None, np.zeros((5, 1)), None)
        assert np.isnan(t).all() and not c.any()
    finally:
        be.close()


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ARG, RANGE = -1, -4
    try:
        rng = np.random.default_rng(62)
        for s in range(4):
            be.belief_write(s, abi.EUCLID1, rng.normal(0, 1, (64, 1)))
        good = lc.desc("linrel_e1_normal", 0, 1)
        prior = lc.desc("prior_e1_normal", 0, -1)
        rows = np.stack([_row(jc.labels(rng, 64, 2), 64), _row(jc.labels(rng, 64, 3), 64)])
        out, cnt = np.full(MAXK * MAXK, 7.0), np.full(2 * MAXK, 7, dtype=np.int32)

        def call(d, ra=0, rb=1, n=1, lab=rows, n_rows=None, o=out, descs=True, context=ctx, rap=True):
            arr = (abi.LikelihoodDesc * 1)(d)
            a, b = np.array([ra], dtype=np.int32), np.array([rb], dtype=np.int32)
            rc = lib.nbp_run_factor_mode_likelihood(context, arr if descs else None, a.ctypes.data_as(ip) if rap else None, b.ctypes.data_as(ip), n,
                                                    lab.ctypes.data_as(ip) if lab is not None else None, len(rows) if n_rows is None else n_rows,
                                                    o.ctypes.data_as(dp) if o is not None else None, cnt.ctypes.data_as(ip))
            assert rc == 0 or (np.all(out == 7.0) and np.all(cnt == 7)), "a refused call leaves the outputs untouched"
            return rc

        def edit(name="linrel_e1_normal", sa=0, sb=1, **kw):
            d = lc.desc(name, sa, sb)
            for k, v in kw.items():
                if k.startswith("comp"):
                    d.comp[int(k[4])][int(k[6:])] = v
                else:
                    setattr(d, k, v)
            return d
        assert call(good, descs=False) == ARG and call(good, o=None) == ARG and call(good, context=None) == ARG and call(good, rap=False) == ARG
        assert call(good, lab=None) == ARG and call(good, n_rows=-1) == ARG
        assert call(good, n=0) == 0 and lib.nbp_run_factor_mode_likelihood(ctx, None, None, None, 0, None, 0, None, None) == 0 and out[0] == 7.0
        # everything nbp_run_factor_likelihood refuses, through the same check (its own test walks the whole list)
        refused = [
            (edit(kind=abi.F_MSGPRIOR), ARG), (edit(kind=abi.F_PASSTHROUGH), ARG), (edit(kind=9), ARG), (edit(comp0_12=float(abi.DIST_TABLE)), ARG),
            (edit("linrel_e2_full", comp0_5=0.25), ARG), (edit(comp0_4=0.0), ARG), (edit("linrel_e1_uniform", comp0_4=np.inf), ARG),
            (edit(ncomp=0), ARG), (edit(ncomp=5), ARG), (edit(comp0_0=-1.0), ARG), (edit(kind=abi.F_SE2), ARG), (edit(manifold=6), ARG),
            (edit("prior_e1_normal", sb=1), ARG), (edit("linrel_e3_full", partial_mask=7), ARG), (edit(partial_mask=2), RANGE),
            (edit(sa=-1), RANGE), (edit(sa=4), RANGE), (edit(sb=4), RANGE), (edit(sb=-1), RANGE),
        ]
        for i, (d, status) in enumerate(refused):
            assert call(d) == status, (i, lib.nbp_last_error())
            assert b"item 0" in lib.nbp_last_error()
        # the rows
        for ra, rb in ((2, 1), (-2, 1), (0, 2), (0, -2)):
            assert call(good, ra=ra, rb=rb) == RANGE and b"item 0" in lib.nbp_last_error(), (ra, rb)
        assert call(good, ra=0, rb=0, n_rows=0) == RANGE
        assert call(prior, ra=0, rb=1) == ARG and b"unary" in lib.nbp_last_error()
        for bad in (MAXK, -2, 1 << 20):
            lab = rows.copy()
            lab[1, 5] = bad
            assert call(good, lab=lab) == ARG and b"label row 1" in lib.nbp_last_error() and b"entry 5" in lib.nbp_last_error()
            assert call(good, ra=0, rb=-1, lab=lab) == 0  # (a row no item names is not read)
            out[:], cnt[:] = 7.0, 7
        with pytest.raises(iif.NbpError, match="-4"):
            be.run_factor_mode_likelihood([good], [0], [5], rows)
        # the host-buffer form
        a = np.ascontiguousarray(rng.normal(0, 1, (10, 1)))
        la = np.zeros(10, dtype=np.int32)
        ap, lp, op = a.ctypes.data_as(dp), la.ctypes.data_as(ip), out.ctypes.data_as(dp)
        f = lib.nbp_factor_mode_likelihood
        assert f(ctx, None, ap, 10, lp, ap, 10, lp, op, None) == ARG and f(ctx, C.byref(good), None, 10, lp, ap, 10, lp, op, None) == ARG
        assert f(ctx, C.byref(good), ap, 10, lp, None, 10, lp, op, None) == ARG and f(ctx, C.byref(good), ap, 10, lp, ap, 10, lp, None, None) == ARG
        assert f(ctx, C.byref(edit(comp0_4=0.0)), ap, 10, lp, ap, 10, lp, op, None) == ARG
        la[3] = MAXK
        assert f(ctx, C.byref(good), ap, 10, lp, ap, 10, None, op, None) == ARG and b"entry 3" in lib.nbp_last_error()
        assert f(ctx, C.byref(good), ap, 10, None, ap, 10, lp, op, None) == ARG and np.all(out == 7.0)
        la[3] = 0
        assert f(ctx, C.byref(good), ap, 10, lp, ap, 10, None, op, None) == 0 and np.isfinite(out[0]) and np.isnan(out[1:]).all()
        assert f(ctx, C.byref(prior), ap, 10, lp, None, 0, None, op, None) == 0 and np.isfinite(out[0])
        # a valid call still works on the same context (the host-buffer calls above left their points in slots 0 and 1)
        out[:] = 7.0
        assert call(good, ra=-1, rb=-1) == 0
        jc.hold(out.reshape(MAXK, MAXK), jc.restate(good, a, None, a, None), "after the refusals")
    finally:
        be.close()


# ---- 6. the mirror -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["ring", "ring without the anchor", "doors"])
def test_joint_modes_equal_the_numpy_route(hip_backend, scene):
    fg = {"ring": jc.ring_graph, "ring without the anchor": lambda: jc.ring_graph(with_cu=False), "doors": jc.doors_graph}[scene]()
    ref = iif.jointModes(fg)
    got = iif.jointModes(fg, backend=hip_backend)
    jc.hold_joint(got, ref, fg, scene)
    assert got.coverage == ref.coverage and all(np.array_equal(got.best_points[v], ref.best_points[v]) or
                                                np.abs(got.best_points[v] - ref.best_points[v]).max() < 1e-6 for v in ref.best)
    if scene == "ring":
        assert got.best_weight > 0.999 and got.logscores[0] - got.logscores[1] > 1000
    if scene == "ring without the anchor":
        assert np.all((got.weights[:2] > 0.4) & (got.weights[:2] < 0.6)) and np.all(got.weights[2:] < 1e-300)
    if scene == "doors":
        assert got.best["x"] == jc.mode_near(got.modes["x"], 2.05)
        one = iif.factorModeLikelihood(fg, "door", modes=got.modes, backend=hip_backend)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one.tables, got.tables["door"].tables))


# ---- 7. the session --------------------------------------------------------------------------------------------------------------------------
def test_session_reads_the_resident_beliefs_where_they_lie(hip_backend):
    """the circular-doors graph (a chain of poses with multihypo sightings of doors): after a solve, the joint hypothesis from one
    run_modes launch and one table launch on the resident beliefs; `stats` does not move; after invalidate(v) exactly that belief
    goes up"""
    fg = iif.generateCircularDoors(nposes=6, N=64, sightEvery=3)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=71)
        before = copy.deepcopy(ses.stats)
        got = ses.jointModes()
        assert ses.stats == before
        host = iif.jointModes(fg, backend=ses.backend)
        assert any(r.hypotheses for r in got.tables.values()), "the graph has multihypo sightings"
        assert got.variables == host.variables and got.best == host.best and got.skipped == host.skipped
        assert np.array_equal(got.combos, host.combos) and list(got.tables) == list(host.tables) and len(got.tables) > 5
        for f in got.tables:
            # the same beliefs on the same device: the session's slots hold what the host copy was read back from
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got.tables[f].tables, host.tables[f].tables)), f
        for v in got.modes:
            assert np.array_equal(got.modes[v].labels, host.modes[v].labels)
        assert np.float64(got.best_logscore).tobytes() == np.float64(host.best_logscore).tobytes() and got.logZ == host.logZ
        ses.invalidate("x3")
        again = ses.jointModes()
        assert ses.stats["uploads"] == before["uploads"] + 1 and ses.stats["readbacks"] == before["readbacks"]
        assert again.best == got.best and np.float64(again.best_logscore).tobytes() == np.float64(got.best_logscore).tobytes()
        assert ses.jointModes().best == got.best and ses.stats["uploads"] == before["uploads"] + 1
