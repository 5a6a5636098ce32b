"""-m gpu: belief overlaps on the device (nbp_run_overlap / nbp_kde_overlap / nbp_run_overlap_search, csrc/nbp_overlap.h) through the C
ABI, the mirror and a solve session.  The pair form is held to the numpy restatement with the tolerance overlap_cases.restate works
out per case on the host: 16 max(|float64 - long double| of the restatement, 4 ulp(max(1, |l|))).  The search is held to the pair form
on the device, exactly: every pair of every scene is evaluated by run_overlap and ranked on the host."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import overlap_cases as oc
import ppe_cases as pc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
ov = iif.overlap


def _full(m):
    return (1 << abi.MANIFOLD_DIM[m]) - 1


def _pairs_against_restatement(be, cases, what):
    """cases = [(ma, A, ha, ka, mb, B, hb, kb)]: pair i in slots 2 i, 2 i + 1; ONE run_overlap; every record held to its restatement"""
    slots, mans, bels = [], [], []
    for i, (ma, A, ha, ka, mb, B, hb, kb) in enumerate(cases):
        slots += [2 * i, 2 * i + 1]
        mans += [ma, mb]
        bels += [(pc.to_points(ma, A), ha, None), (pc.to_points(mb, B), hb, None)]
    be.beliefs_write(slots, mans, bels)
    recs = be.run_overlap(slots[0::2], slots[1::2], mans[0::2], mans[1::2], [c[3] for c in cases], [c[7] for c in cases])
    worst = 0.0
    for i, c in enumerate(cases):
        ref = oc.restate(c[0], bels[2 * i][0], c[2], c[3], c[4], bels[2 * i + 1][0], c[6], c[7])  # (the host points the device was given)
        worst = max(worst, oc.hold(recs[i], ref, f"{what} pair {i} (m{c[0]} k{c[3]} n{len(c[1])} | m{c[4]} k{c[7]} n{len(c[5])})"))
    print(f"{what}: {len(cases)} pairs, largest error / tolerance {worst:.3f}")
    return recs


# ---- 1. the pair form against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 200, 257, 512])
def test_every_manifold_at_full_count(hip_backend, N):
    rng = np.random.default_rng(100 + N)
    cases = [(m, oc.cloud("gaussian", m, N, rng), oc.bandwidth(m), _full(m), m, oc.cloud("gaussian", m, N, rng, 0.4), oc.bandwidth(m, 0.7), _full(m))
             for m in oc.MANIFOLDS]
    be = hip_backend(N, 2 * len(cases))
    try:
        _pairs_against_restatement(be, cases, f"N={N}")
    finally:
        be.close()


def test_every_admissible_pair_of_masks(hip_backend):
    """all 99 ordered pairs of (manifold, mask), SE(2)(x, y) against Euclid(2) among them, in one launch"""
    rng = np.random.default_rng(200)
    cases = [(ma, oc.cloud("gaussian", ma, 64, rng), oc.bandwidth(ma), ka, mb, oc.cloud("gaussian", mb, 50, rng, 0.3), oc.bandwidth(mb, 1.3), kb)
             for (ma, ka), (mb, kb) in oc.ADMISSIBLE]
    assert ((abi.SE2, 3), (abi.EUCLID2, 3)) in oc.ADMISSIBLE
    be = hip_backend(64, 2 * len(cases))
    try:
        _pairs_against_restatement(be, cases, "masks")
    finally:
        be.close()


@pytest.mark.parametrize("counts", [(1, 2), (2, 63), (63, 64), (64, 65), (65, 200), (200, 1)])
def test_counts_below_the_context_size(hip_backend, counts):
    rng = np.random.default_rng(300 + counts[0])
    cases = [(m, oc.cloud("gaussian", m, counts[0], rng), oc.bandwidth(m), _full(m), m, oc.cloud("bimodal", m, counts[1], rng, 0.2), oc.bandwidth(m, 0.8),
              _full(m)) for m in (abi.EUCLID2, abi.CIRCULAR, abi.SE2)]
    be = hip_backend(200, 2 * len(cases))
    try:
        _pairs_against_restatement(be, cases, f"counts {counts}")
    finally:
        be.close()


@pytest.mark.parametrize("kind", oc.CLOUDS)
def test_clouds(hip_backend, kind):
    """Gaussian, bimodal, all-identical and far-apart clouds on every manifold; far apart, logc is finite where every density
    underflows"""
    rng = np.random.default_rng(400)
    cases = [(m, oc.cloud(kind, m, 200, rng), oc.bandwidth(m), _full(m), m, oc.cloud("gaussian", m, 150, rng, 0.5), oc.bandwidth(m, 0.6), _full(m))
             for m in oc.MANIFOLDS]
    be = hip_backend(200, 2 * len(cases))
    try:
        recs = _pairs_against_restatement(be, cases, kind)
        assert np.all(np.isfinite(recs))
        if kind == "far":
            assert all(-3e6 < recs[i, 0] < -1e5 for i, m in enumerate(oc.MANIFOLDS) if m != abi.CIRCULAR)
    finally:
        be.close()


# ---- 2. the pair form, exact -------------------------------------------------------------------------------------------------------------
def test_copies_same_slot_and_bad_bandwidths(hip_backend):
    be = hip_backend(200, 12)
    try:
        rng = np.random.default_rng(500)
        for m in oc.MANIFOLDS:
            X, h = pc.to_points(m, oc.cloud("bimodal", m, 130, rng)), oc.bandwidth(m)
            be.beliefs_write([0, 1, 2], [m] * 3, [(X, h, None), (X.copy(), h.copy(), None), (pc.to_points(m, oc.cloud("gaussian", m, 90, rng)), h, None)])
            r = be.run_overlap([0, 0, 0, 2], [1, 0, 2, 0], [m] * 4, [m] * 4, [_full(m)] * 4, [_full(m)] * 4)
            assert r[0, 0] == 0.0 and r[1, 0] == 0.0 and r[0].tobytes() == r[1].tobytes(), (m, r)
            assert r[0, 1] == r[0, 2] == r[0, 3]
            # swapping the roles swaps the self terms bit for bit; the cross terms agree within the restatement's tolerance
            assert r[2, 2] == r[3, 3] and r[2, 3] == r[3, 2] and r[2, 2] == r[0, 2]
            # the host-buffer form is the resident form bit for bit
            got = be.kde_overlap(m, X, h, _full(m), m, pc.to_points(m, oc.cloud("gaussian", m, 90, np.random.default_rng(1))), h, _full(m))
            res = be.run_overlap([0], [1], [m], [m], [_full(m)], [_full(m)])  # (kde_overlap left its beliefs in slots 0 and 1)
            assert got.tobytes() == res[0].tobytes() and np.all(np.isfinite(got))
            for bad in (0.0, -1.0, np.inf, np.nan):
                hx = h.copy()
                hx[-1] = bad
                be.belief_write(3, m, X, hx)
                r = be.run_overlap([3, 2, 0], [2, 3, 2], [m] * 3, [m] * 3, [_full(m)] * 3, [_full(m)] * 3)
                assert np.all(np.isnan(r[:2])) and np.all(np.isfinite(r[2])), (m, bad, r)
                if abi.MANIFOLD_DIM[m] > 1:  # outside the mask the entry is not read
                    assert np.all(np.isfinite(be.run_overlap([3], [2], [m], [m], [1], [1])))
    finally:
        be.close()


def test_300_pairs_in_one_launch_twice(hip_backend):
    """more workgroups than the chip has compute units; a record depends on its pair alone, and two runs are byte-identical"""
    be = hip_backend(100, 12)
    try:
        rng = np.random.default_rng(600)
        mans = [abi.EUCLID2, abi.EUCLID2, abi.SE2, abi.SE2, abi.CIRCULAR, abi.CIRCULAR, abi.EUCLID3, abi.EUCLID3, abi.EUCLID1, abi.EUCLID1, abi.SE2, abi.EUCLID2]
        be.beliefs_write(list(range(12)), mans, [(pc.to_points(m, oc.cloud("gaussian", m, 100 - 3 * i, rng)), oc.bandwidth(m), None) for i, m in enumerate(mans)])
        base = [(0, 1, 3, 3), (2, 3, 7, 7), (4, 5, 1, 1), (6, 7, 7, 7), (8, 9, 1, 1), (10, 11, 3, 3), (2, 4, 4, 1), (8, 6, 1, 2)]
        order = [0] + [(5 * k) % len(base) for k in range(1, 299)] + [0]
        cols = [[base[i][0] for i in order], [base[i][1] for i in order], [mans[base[i][0]] for i in order], [mans[base[i][1]] for i in order],
                [base[i][2] for i in order], [base[i][3] for i in order]]
        r1, r2 = be.run_overlap(*cols), be.run_overlap(*cols)
        assert len(r1) == 300 and r1.tobytes() == r2.tobytes() and np.all(np.isfinite(r1))
        single = [be.run_overlap([a], [b], [mans[a]], [mans[b]], [ka], [kb])[0] for a, b, ka, kb in base]
        for k, i in enumerate(order):
            assert r1[k].tobytes() == single[i].tobytes(), (k, i)
    finally:
        be.close()


# ---- 3. the search against the pair form on the device, exact ----------------------------------------------------------------------------
def _search_equals_pairs(be, scene, topk, min_coeff=ov.MIN_COEFF, reach=ov.REACH, what=""):
    slots, mans, masks = oc.write_scene(be, scene)
    V = len(scene)
    idx, val, found, evaluated = be.run_overlap_search(slots, mans, masks, topk, min_coeff, reach)
    again = be.run_overlap_search(slots, mans, masks, topk, min_coeff, reach)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((idx, val, found, evaluated), again))
    # every pair in canonical order (a = the lower list index), and every belief against itself for its validity
    ii, jj = np.triu_indices(V, 1)
    ii, jj = np.r_[ii, np.arange(V)].astype(int), np.r_[jj, np.arange(V)].astype(int)
    recs = be.run_overlap([slots[i] for i in ii], [slots[j] for j in jj], [mans[i] for i in ii], [mans[j] for j in jj],
                          [masks[i] for i in ii], [masks[j] for j in jj])
    logc = np.full((V, V), np.nan)
    logc[ii, jj] = recs[:, 0]
    logc[jj, ii] = recs[:, 0]
    valid = ~np.isnan(np.diag(logc))
    assert np.all(np.diag(logc)[valid] == 0.0)
    # the host box rule on the points as read back
    back = be.beliefs_read(slots, mans)
    parts = [ov._masked(m, p, bw, k, np.float64) for (p, bw, _), m, k in zip(back, mans, masks)]
    lo, hi = [p[0].min(axis=0) for p in parts], [p[0].max(axis=0) for p in parts]
    logmin, n_pruned = math.log(min_coeff), 0
    for i in range(V):
        if not valid[i]:
            assert found[i] == -1 and evaluated[i] == 0 and np.all(idx[i] == -1) and np.all(np.isneginf(val[i])), (what, i)
            continue
        cands = [(j, logc[i, j]) for j in range(V) if j != i and valid[j]]  # (no pair is left out: the pruned ones too)
        want_idx, want_val, want_found = ov.rank_row(cands, topk, logmin)
        assert np.array_equal(idx[i], want_idx) and val[i].tobytes() == want_val.tobytes() and found[i] == want_found, (what, i, idx[i], want_idx)
        kept = sum(1 for j, _ in cands if not ov.box_skips(lo[i], hi[i], parts[i][1], lo[j], hi[j], parts[j][1], parts[i][2], reach))
        n_pruned += len(cands) - kept
        assert evaluated[i] == kept, (what, i, evaluated[i], kept)
    print(f"{what}: V = {V}, {n_pruned} of {V * (V - 1)} ordered pairs pruned, found per row min {found.min()} max {found.max()}")
    return idx, val, found, evaluated, n_pruned


@pytest.mark.parametrize("V", [1, 2, 3])
def test_search_of_one_two_and_three_beliefs(hip_backend, V):
    be = hip_backend(64, 4)
    try:
        rng = np.random.default_rng(700)
        scene = [(abi.EUCLID2, rng.normal([0.5 * i, 0.0], 0.3, (64 - i, 2)), np.array([0.15, 0.15]), 3) for i in range(V)]
        idx, _, found, evaluated, _ = _search_equals_pairs(be, scene, 8, what=f"V={V}")
        assert found.tolist() == [V - 1] * V and evaluated.tolist() == [V - 1] * V
    finally:
        be.close()


def test_search_of_a_chain_that_returns_to_its_start(hip_backend):
    scene = oc.loop_chain(300, 64)
    be = hip_backend(64, 300)
    try:
        idx, _, found, evaluated, n_pruned = _search_equals_pairs(be, scene, 8, what="loop of 300")
        assert 299 in idx[0] and 0 in idx[299]  # the loop closure, in the lists of both ends
        assert n_pruned > 0.9 * 300 * 299 and evaluated.max() < 30
    finally:
        be.close()


def test_search_mixes_poses_and_landmarks_on_x_and_y(hip_backend):
    scene = oc.poses_and_landmarks(64)
    be = hip_backend(64, len(scene))
    try:
        idx, _, found, _, n_pruned = _search_equals_pairs(be, scene, 8, what="40 poses + 20 landmarks")
        assert n_pruned > 0 and any(j >= 40 for j in idx[0]) and any(0 <= j < 40 for j in idx[40])  # pose 0 and landmark 0 see each other
    finally:
        be.close()


def test_search_of_circular_beliefs_prunes_nothing(hip_backend):
    scene = oc.circular_beliefs(40, 64)
    be = hip_backend(64, 40)
    try:
        _, _, _, evaluated, n_pruned = _search_equals_pairs(be, scene, 8, what="40 circular")
        assert n_pruned == 0 and evaluated.tolist() == [39] * 40
    finally:
        be.close()


def test_search_rows_with_0_k_minus_1_k_and_k_plus_1_partners_ties_and_a_bad_bandwidth(hip_backend):
    k = 3
    scene = oc.clusters(k, 64)
    be = hip_backend(64, len(scene) + 1)
    try:
        idx, val, found, _, _ = _search_equals_pairs(be, scene, k, what="clusters")
        assert sorted(set(found.tolist())) == [0, k - 1, k, k + 1]
        ties = [i for i in range(len(scene)) if found[i] > 0 and val[i, 0] == 0.0]
        assert len(ties) == 3  # the three bit-identical copies: each has the other two at logc == 0.0, the lower index first
        for i in ties:
            assert val[i, 1] == 0.0 and idx[i, 0] < idx[i, 1] and set(idx[i, :2]) | {i} == set(ties)
        others = [i for i in range(len(scene)) if found[i] == k + 1 and i not in ties]
        for i in others:  # every other belief of that cluster ties on the copies: ascending list index among equals
            rows = [r for r in range(k) if idx[i, r] in ties]
            assert len({val[i, r] for r in rows}) == 1 and [idx[i, r] for r in rows] == sorted(idx[i, r] for r in rows)
        bad = scene + [(abi.EUCLID2, scene[0][1] + 0.1, np.array([0.15, 0.0]), 3)]
        idx2, val2, found2, evaluated2, _ = _search_equals_pairs(be, bad, k, what="clusters + a bad bandwidth")
        assert found2[-1] == -1 and evaluated2[-1] == 0 and not np.any(idx2 == len(scene))
        assert idx2[:-1].tobytes() == idx.tobytes() and val2[:-1].tobytes() == val.tobytes()
    finally:
        be.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_index_and_leave_the_context_usable(hip_backend):
    be = hip_backend(64, 4)
    try:
        rng = np.random.default_rng(800)
        mans = [abi.EUCLID2, abi.SE2, abi.CIRCULAR, abi.EUCLID2]
        be.beliefs_write([0, 1, 2, 3], mans, [(pc.to_points(m, oc.cloud("gaussian", m, 64, rng)), oc.bandwidth(m), None) for m in mans])
        E2, SE2, CI = abi.EUCLID2, abi.SE2, abi.CIRCULAR
        good = ([0, 0], [3, 1], [E2, E2], [E2, SE2], [3, 3], [3, 3])

        def pair(pos, value, match):
            cols = [list(c) for c in good]
            cols[pos][1] = value
            with pytest.raises(iif.NbpError, match=match):
                be.run_overlap(*cols)
        pair(5, 5, r"status -1.*belief 1.*inadmissible")        # (x, y) against (x, theta)
        pair(5, 1, r"status -1.*belief 1.*inadmissible")        # two coordinates against one
        pair(4, 0, r"status -4.*belief 1.*empty mask")
        pair(5, 8, r"status -4.*belief 1.*outside the manifold")
        pair(4, 4, r"status -4.*belief 1.*outside the manifold")
        pair(1, 4, r"status -4.*belief 1.*slot out of range")
        pair(0, -1, r"status -4.*belief 1.*slot out of range")
        pair(3, 9, r"status -1.*belief 1.*unknown manifold")
        with pytest.raises(iif.NbpError, match=r"status -4.*belief 0.*empty mask"):
            be.kde_overlap(E2, np.zeros((3, 2)), [0.1, 0.1], 0, E2, np.zeros((3, 2)), [0.1, 0.1], 3)
        with pytest.raises(iif.NbpError, match=r"status -1.*inadmissible"):
            be.kde_overlap(E2, np.zeros((3, 2)), [0.1, 0.1], 1, CI, np.zeros((3, 1)), [0.1], 1)
        ok = be.run_overlap(*good)
        assert np.all(np.isfinite(ok))

        def search(match, slots=(0, 3, 1), ms=(E2, E2, SE2), ks=(3, 3, 3), **kw):
            with pytest.raises(iif.NbpError, match=match):
                be.run_overlap_search(list(slots), list(ms), list(ks), **kw)
        search(r"status -1.*belief 2.*not admissible", ks=(3, 3, 5))
        search(r"status -1.*belief 1.*not admissible", slots=(0, 2, 1), ms=(E2, CI, SE2), ks=(1, 1, 1))
        search(r"status -4.*belief 2.*empty mask", ks=(3, 3, 0))
        search(r"status -4.*belief 1.*outside the manifold", ks=(3, 4, 3))
        search(r"status -4.*belief 2.*slot out of range", slots=(0, 3, 4))
        search(r"status -4.*topk", topk=0)
        search(r"status -4.*topk", topk=17)
        search(r"status -4.*log\(min_coeff\)", reach=2.0)
        search(r"status -4.*log\(min_coeff\)", min_coeff=1e-9)
        search(r"status -1.*reach", reach=float("nan"))
        search(r"status -1.*min_coeff", min_coeff=0.0)
        idx, val, found, evaluated = be.run_overlap_search([0, 3, 1], [E2, E2, SE2], [3, 3, 3], topk=16)
        assert idx.shape == (3, 16) and np.all(found >= 0) and be.run_overlap(*good).tobytes() == ok.tobytes()
    finally:
        be.close()


def test_every_refusal_of_the_kde_form_comes_before_slots_0_and_1_are_touched(hip_backend):
    be = hip_backend(64, 2)
    try:
        E2, CI, rng = abi.EUCLID2, abi.CIRCULAR, np.random.default_rng(801)
        kept = [(np.ascontiguousarray(pc.cloud("gaussian", E2, 64, rng)), np.array([0.3, 0.2 + 0.1 * s])) for s in (0, 1)]
        for s, (p, h) in enumerate(kept):
            be.belief_write(s, E2, p, h)
        before = [be.belief_read(s, E2) for s in (0, 1)]
        a, h2, c1, h1 = np.ones((64, 2)), np.array([0.5, 0.5]), np.ones((64, 1)), np.array([0.5])

        def refused(code, text, call):
            with pytest.raises(iif.NbpError) as e:
                call()
            assert str(e.value) == f"libnbp status {code}: {text}", e.value
        for ka, kb in ((0, 3), (3, 0)):
            refused(-4, "overlap: belief 0: empty mask", lambda: be.kde_overlap(E2, a, h2, ka, E2, a, h2, kb))
        for ka, kb in ((4, 3), (3, 4), (-1, 3), (3, -1)):
            refused(-4, "overlap: belief 0: coordinate outside the manifold", lambda: be.kde_overlap(E2, a, h2, ka, E2, a, h2, kb))
        refused(-1, "overlap: belief 0: inadmissible pair: the masked coordinates differ in number or kind",
                lambda: be.kde_overlap(CI, c1, h1, 1, E2, a, h2, 1))
        refused(-1, "overlap: belief 0: inadmissible pair: the masked coordinates differ in number or kind",
                lambda: be.kde_overlap(E2, a, h2, 3, E2, a, h2, 1))
        dp, rec = C.POINTER(C.c_double), abi.OverlapRec()  # (the wrapper cannot shape the points of a manifold it does not know)
        refused(-1, "overlap: unknown manifold", lambda: be._check(be.lib.nbp_kde_overlap(
            be._ctx, E2, a.ctypes.data_as(dp), 64, h2.ctypes.data_as(dp), 3, 9, a.ctypes.data_as(dp), 64, h2.ctypes.data_as(dp), 3, C.byref(rec))))
        for s, (p, h) in enumerate(kept):
            after = be.belief_read(s, E2)
            assert after[0].tobytes() == p.tobytes() and after[1].tobytes() == h.tobytes(), s
            assert all(x.tobytes() == y.tobytes() for x, y in zip(after, before[s])), s
        assert np.isfinite(be.kde_overlap(E2, a, h2, 1, E2, a, h2, 2)).all()  # the context stays usable
    finally:
        be.close()


# ---- 5. the mirror and the session ---------------------------------------------------------------------------------------------------------
def test_session_finds_the_overlaps_of_resident_beliefs_without_moving_them(hip_backend):
    fg = iif.generateChainEuclid(24, vardims=2, priorEvery=8, N=200)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=81)
        before = copy.deepcopy(ses.stats)
        got = ses.findOverlaps()
        pairs = ses.overlapVariables([("x3", "x4"), ("x4", "x3"), ("x0", "x23")])
        assert ses.stats == before  # no belief travelled
        labels = list(ses._labels)
        want = iif.findOverlaps(fg, labels, backend=hip_backend)
        assert list(got) == labels and len(got) == 24
        assert got.idx.tobytes() == want.idx.tobytes() and got.logc.tobytes() == want.logc.tobytes()
        assert got.n_found == want.n_found and got.n_evaluated == want.n_evaluated and got.pairs() == want.pairs()
        want_pairs = iif.overlapVariables(fg, list(pairs), backend=hip_backend)
        assert pairs == want_pairs
        # neighbours of a unit-spaced chain with sigma 0.1 per step: what a pose overlaps with is a pose beside it
        for v, row in got.items():
            i = int(v[1:])
            print(f"{v}: found {got.n_found[v]} evaluated {got.n_evaluated[v]} {[(u, round(c, 4)) for u, c in row]}")
            assert got.n_evaluated[v] < 23 and all(abs(int(u[1:]) - i) <= 3 for u, _ in row) and all(1e-3 <= c <= 1.0 + 1e-12 for _, c in row)
        assert all(a != b and got.labels.index(a) < got.labels.index(b) for a, b, _ in got.pairs())
        assert pairs[("x0", "x23")].coeff < 1e-3 and np.isfinite(pairs[("x0", "x23")].logcoeff)
        sub = ses.findOverlaps(["x2", "x3", "x9"], dims=(1,), number=2)
        assert list(sub) == ["x2", "x3", "x9"] and ses.stats == before
        one = iif.beliefOverlap(iif.getBelief(fg, "x3"), iif.getBelief(fg, "x4"), iif.ContinuousEuclid(2), backend=hip_backend)
        assert one == pairs[("x3", "x4")]
        with pytest.raises(ValueError):
            ses.findOverlaps(reach=2.0)
        with pytest.raises(ValueError):
            ses.findOverlaps(["x1", "nobody"])
