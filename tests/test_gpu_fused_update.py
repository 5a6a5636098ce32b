"""-m gpu: the fused variable-update kernel (csrc/nbp_fused.h: proposals, their bandwidth fits, KD trees, product and the
fit of the result in one workgroup per variable) against the oracle and against the three-launch form of the same round
(proposal kernel -> prep kernel -> product kernel).  All three run the same operations with the same random streams and
one summation order (round 6), so the comparison is `np.array_equal` -- no tolerance -- on the points, the bandwidth and
infoPerCoord of every output slot and of every proposal slot the program leaves written, and on the counters between the
two device forms.  The cases are those of tests/fused_cases.py (its docstring lists what the planner accepts and what it
refuses); tests/test_fused_cases.py runs them on the oracle alone.

Sizes: every (N, F) of fused_cases.SIZES x SIZE_F lies under the LDS ceiling of nbp_program_finalize (158 KiB; N = 256
with F = 4 needs 111 232 bytes) and must fuse -- none falls back; N = 257 and N = 512 (Npad > 256) are refused."""
import os

import numpy as np
import pytest

import fused_cases as fc
from fused_cases import legacy_round as _round  # (test_gpu_product_first_label.py imports it from here)
from parity_utils import abi, assert_points_close, iif, rand_points

pytestmark = pytest.mark.gpu

N, MAN = 200, abi.EUCLID2


@pytest.fixture
def fused_min():
    """smallest stage that runs fused, for contexts created inside the test"""
    old = os.environ.get("NBP_FUSED_MIN")

    def set_(n):
        os.environ["NBP_FUSED_MIN"] = str(n)

    yield set_
    if old is None:
        os.environ.pop("NBP_FUSED_MIN", None)
    else:
        os.environ["NBP_FUSED_MIN"] = old


def _run_round(hip_backend, nops, F, fused, lazy=False, read=(0, -1)):
    rng = np.random.default_rng(5)
    a, b, c = rand_points(rng, MAN, N, 0.0, 0.4), rand_points(rng, MAN, N, 2.0, 0.4), rand_points(rng, MAN, N, 1.0, 0.6)
    props, prods, stride = _round(nops, F)
    be = hip_backend(N, 4 + stride * nops, 0)
    for s, p in enumerate((a, b, c)):
        be.slot_write(s, MAN, p)
    prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)], lazy_bandwidth=lazy, fused_updates=fused)
    nf = prog.num_fused()
    prog.run()
    be.synchronize()
    out = []
    for i in read:
        i = i % nops
        out.append(be.belief_read(4 + stride * i + F, MAN))
    prop0 = be.belief_read(4, MAN)  # the first proposal's own slot: written when the program ends with it still there
    diag = be.diag()
    prog.close()
    be.close()
    return nf, out, prop0, diag


@pytest.mark.parametrize("F", [1, 2, 3, 4])
def test_fused_round_equals_three_launch_round(hip_backend, fused_min, F):
    fused_min(256)
    nops = 1100
    nf, fo, fp, fd = _run_round(hip_backend, nops, F, True)
    nu, uo, up, ud = _run_round(hip_backend, nops, F, False)
    assert nf == 1 and nu == 0
    for (p, bw, ipc), (q, bw2, ipc2) in zip(fo, uo):
        assert_points_close(MAN, q, p, rtol=0, what=f"fused product, F = {F}")
        np.testing.assert_allclose(bw, bw2, rtol=0)
        np.testing.assert_array_equal(ipc, ipc2)
    # proposals that are still in their slots when the program ends are written there by the fused kernel too
    assert_points_close(MAN, up[0], fp[0], rtol=0, what="proposal slot")
    if F > 1:  # (a lone proposal's fit travels with the pass-through product: its own slot keeps no bandwidth)
        np.testing.assert_allclose(fp[1], up[1], rtol=0)
    for k in ("solves", "nonconverged", "nan_results", "residual_evals"):
        assert fd[k] == ud[k], k


def test_small_rounds_keep_the_three_launch_form(hip_backend, fused_min):
    fused_min(256)
    nf, _, _, _ = _run_round(hip_backend, 100, 2, True)
    assert nf == 0


def test_fused_round_against_the_oracle(oracle_backend, hip_backend, fused_min):
    fused_min(16)
    nops, F = 24, 3
    rng = np.random.default_rng(9)
    pts = [rand_points(rng, MAN, N, c, 0.4) for c in (0.0, 2.0, 1.0)]
    props, prods, stride = _round(nops, F)
    res = []
    for make in (oracle_backend, hip_backend):
        be = make(N, 4 + stride * nops, 0)
        for s, p in enumerate(pts):
            be.slot_write(s, MAN, p)
        prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)])
        if make is hip_backend:
            assert prog.num_fused() == 1
        prog.run()
        be.synchronize()
        res.append([be.slot_read(4 + stride * i + F, MAN) for i in range(nops)])
        prog.close()
        be.close()
    for (p, bw), (q, bw2) in zip(*res):
        assert_points_close(MAN, p, q, rtol=0, what="fused update vs oracle")
        np.testing.assert_allclose(bw2, bw, rtol=0)


def test_later_readers_of_a_proposal_slot_see_it(hip_backend, fused_min):
    """a stage behind the fused pair that reads a proposal from its arena slot (here: a slot copy) gets the proposal"""
    fused_min(64)
    nops, F = 300, 2
    rng = np.random.default_rng(2)
    pts = [rand_points(rng, MAN, N, c, 0.4) for c in (0.0, 2.0, 1.0)]
    props, prods, stride = _round(nops, F)
    extra = 4 + stride * nops
    outs = []
    for fused in (True, False):
        be = hip_backend(N, extra + 2, 0)
        for s, p in enumerate(pts):
            be.slot_write(s, MAN, p)
        copies = [abi.CopyDesc(4 + stride * 7, extra), abi.CopyDesc(4 + stride * 7 + 1, extra + 1)]
        prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods), (abi.STAGE_COPIES, copies)], fused_updates=fused)
        assert prog.num_fused() == (1 if fused else 0)
        prog.run()
        be.synchronize()
        outs.append([be.slot_read(extra, MAN), be.slot_read(extra + 1, MAN)])
        prog.close()
        be.close()
    for (p, bw), (q, bw2) in zip(*outs):
        assert_points_close(MAN, q, p, rtol=0, what="copied proposal")
        np.testing.assert_allclose(bw, bw2, rtol=0)
        assert np.abs(p).max() > 0


def test_a_range_that_splits_a_fused_pair_runs_it_in_three_launches(hip_backend, fused_min):
    """nbp_program_run(first, last) with a range that ends or starts between the two stages of a fused pair (legal when the
    program was finalized; round 4 refused it with NBP_ERR_ARG): the pair runs in the three-launch form -- the proposals
    to their arena slots with their fits at the end of the range, then KD builds, products and the fits of the results.
    The same particles and bandwidths as a program with fused updates off, run in the same two halves."""
    fused_min(64)
    nops, F = 200, 2
    props, prods, stride = _round(nops, F)
    rng = np.random.default_rng(5)
    pts = [rand_points(rng, MAN, N, c, 0.4) for c in (0.0, 2.0, 1.0)]
    res = []
    for fused in (True, False):
        be = hip_backend(N, 4 + stride * nops, 0)
        for s, p_ in enumerate(pts):
            be.slot_write(s, MAN, p_)
        prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)], fused_updates=fused)
        assert prog.num_fused() == (1 if fused else 0)
        prog.run(0, 1)
        be.synchronize()
        mid = [be.belief_read(4 + stride * i + j, MAN) for i in (0, 77, nops - 1) for j in range(F)]  # the proposals, fitted
        prog.run(1, 2)
        be.synchronize()
        out = [be.belief_read(4 + stride * i + F, MAN) for i in (0, 77, nops - 1)]
        prog.close()
        be.close()
        res.append((mid, out))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert_points_close(MAN, a[0], b[0], rtol=0, what="split fused pair vs three-launch program")
        np.testing.assert_allclose(a[1], b[1], rtol=0)  # bandwidths
        np.testing.assert_allclose(a[2], b[2])             # infoPerCoord
        assert np.all(a[1] > 0)


def test_whole_solve_with_fused_rounds(oracle_backend, hip_backend, monkeypatch):
    """a chain solved with every round of >= 16 updates fused, the same solve in the three-launch form and the oracle's solve
    of the same graph and seed: every variable particle-identical among the three (and at the truth)"""
    monkeypatch.setenv("NBP_FUSED_MIN", "16")
    fused_rounds = []
    close = iif.backend.HipProgram.close

    def counting_close(prog):
        if prog._p:
            fused_rounds.append(prog.num_fused())
        close(prog)

    monkeypatch.setattr(iif.backend.HipProgram, "close", counting_close)

    def solve(backend, fused=True):
        if not fused:
            monkeypatch.setenv("NBP_NO_FUSED_UPDATE", "1")
        try:
            fg, order = fc.chain_graph()
            iif.solveTree(fg, eliminationOrder=order, backend=backend, seed=3)
        finally:
            monkeypatch.delenv("NBP_NO_FUSED_UPDATE", raising=False)
        return {v: (fg.getVal(v), fg.getVariable(v).bw) for v in fg.ls()}

    a = solve(hip_backend)  # (a solve closes two programs: graph initialisation, then the tree)
    nfused = sum(fused_rounds)
    assert nfused >= 1, fused_rounds
    del fused_rounds[:]
    b = solve(hip_backend, fused=False)
    assert fused_rounds and sum(fused_rounds) == 0, fused_rounds
    o = solve(oracle_backend)
    print(f"whole solve: {nfused} fused rounds")
    for i, v in enumerate(sorted(a, key=lambda s: int(s[1:]))):
        assert np.abs(a[v][0].mean(axis=0) - i).max() < 0.6, (v, a[v][0].mean(axis=0))
        for other, what in ((b, "three-launch solve"), (o, "oracle's solve")):
            assert np.array_equal(a[v][0], other[v][0]), f"{v}: points differ from the {what}"
            assert np.array_equal(a[v][1], other[v][1]), f"{v}: bandwidth differs from the {what}"


# ---- the cases of fused_cases.py: fused form == three-launch form == oracle --------------------------------------------------
def _set_form(monkeypatch, form):
    monkeypatch.setenv("NBP_FUSED_MIN", "16")  # (read when the context is created)
    if form == "p1":
        monkeypatch.setenv("NBP_FUSED_P1_MIN", "1")  # one lane per particle, the form of rounds that fill the chip


@pytest.fixture(scope="module")
def refs(oracle_backend, hip_backend):
    """case -> (the oracle's result, the three-launch form's): computed once per case and shared by the two forms of the
    kernel (fused_updates = False: neither depends on NBP_FUSED_MIN / NBP_FUSED_P1_MIN)"""
    done = {}

    def get(case):
        if case.name not in done:
            done[case.name] = (case.run(oracle_backend), case.run(hip_backend, fused=False))
        return done[case.name]

    return get


def _same(case, got, ref, what, lazy=False):
    for k, ((p, bw, ipc), (q, bw2, ipc2)) in enumerate(zip(got["out"], ref["out"])):
        assert np.array_equal(p, q), f"{case.name}: output {k}: points differ from {what}"
        assert np.array_equal(bw, bw2), f"{case.name}: output {k}: bandwidth differs from {what}"
        assert np.array_equal(ipc, ipc2), f"{case.name}: output {k}: infoPerCoord differs from {what}"
    # the proposals are still in their slots when the program ends: written there by either form.  (A lone proposal's fit
    # travels with the pass-through product, a proposal nothing reads is not fitted under lazy_bandwidth: no bandwidth then)
    for k, ((p, bw, ipc), (q, bw2, ipc2)) in enumerate(zip(got["prop"], ref["prop"])):
        assert np.array_equal(p, q), f"{case.name}: proposal {k}: points differ from {what}"
        assert np.array_equal(ipc, ipc2), f"{case.name}: proposal {k}: infoPerCoord differs from {what}"
        if case.F > 1 and not lazy:
            assert np.array_equal(bw, bw2), f"{case.name}: proposal {k}: bandwidth differs from {what}"
    assert np.array_equal(got["side"], ref["side"]), f"{case.name}: recorded hypotheses / labels differ from {what}"


def _check(case, want_fused, refs, hip_backend):
    orc, three = refs(case)
    got = case.run(hip_backend)
    assert three["nf"] == 0
    assert got["nf"] == want_fused, f"{case.name}: {got['nf']} fused rounds, expected {want_fused}"
    _same(case, three, orc, "the oracle (three-launch form)", case.lazy)
    _same(case, got, orc, "the oracle", case.lazy)
    _same(case, got, three, "the three-launch form", case.lazy)
    for k in ("solves", "nonconverged", "nan_results", "residual_evals"):
        assert got["diag"][k] == three["diag"][k], k
    return got


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("F", fc.SIZE_F)
@pytest.mark.parametrize("N", fc.SIZES)
def test_every_size_equals_the_oracle(N, F, form, refs, hip_backend, monkeypatch):
    """the library's minimum N, every Npad with and without idle lanes, the ceiling N = 256: the round fuses wherever
    nbp_update_lds_bytes admits it -- at every one of these sizes, none falls back -- and gives the oracle's bits"""
    _set_form(monkeypatch, form)
    admitted = fc.admits(N, F)
    print(f"N = {N}, F = {F}: {fc.lds_bytes(max(F, 2), 2, N, fc.npad(N), 2)} bytes of LDS, {'fused' if admitted else 'falls back to three launches'}")
    _check(fc.size_case(N, F), 1 if admitted else 0, refs, hip_backend)


@pytest.mark.parametrize("F", fc.SIZE_F)
@pytest.mark.parametrize("N", fc.SIZES_REFUSED)
def test_more_than_256_particles_keep_the_three_launch_form(N, F, refs, hip_backend, monkeypatch):
    _set_form(monkeypatch, "p2")
    assert not fc.admits(N, F)
    _check(fc.size_case(N, F), 0, refs, hip_backend)


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("N", fc.CLASS_N)
@pytest.mark.parametrize("feature", list(fc.ACCEPTED))
def test_every_accepted_input_class_equals_the_oracle(feature, N, F, form, refs, hip_backend, monkeypatch):
    """one round per descriptor feature that proposals_uniform_class / fused_plan keep fused (fused_cases.ACCEPTED)"""
    _set_form(monkeypatch, form)
    _check(fc.accepted_case(feature, N, F), 1, refs, hip_backend)


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("N", fc.CLASS_N)
@pytest.mark.parametrize("feature", list(fc.ACCEPTED_F1))
def test_single_density_updates_equal_the_oracle(feature, N, form, refs, hip_backend, monkeypatch):
    """F = 1, the early return of the kernel: count and bandwidth handed on, infoPerCoord = ones -- skip_bandwidth, a
    MsgPrior, a nullhypo prior, a mixture, a lone pass-through (full, or resampled to N)"""
    _set_form(monkeypatch, form)
    got = _check(fc.accepted_f1_case(feature, N), 1, refs, hip_backend)
    assert all(np.array_equal(ipc, [1.0, 1.0]) for _, _, ipc in got["out"])


@pytest.mark.parametrize("N", fc.CLASS_N)
@pytest.mark.parametrize("feature", list(fc.REFUSED))
def test_every_refused_input_class_keeps_the_three_launch_form(feature, N, refs, hip_backend, monkeypatch):
    """one round per feature fused_plan refuses (fused_cases.REFUSED): no fused round, the oracle's bits all the same"""
    _set_form(monkeypatch, "p2")
    _check(fc.refused_case(feature, N), 0, refs, hip_backend)


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("cnt", fc.BELOW)
def test_operands_with_fewer_than_n_points(cnt, form, refs, hip_backend, monkeypatch):
    """the relative's other variable and the MsgPrior's KDE hold 1, 2, 63, 150 of N = 200 points: `anyn_index` and the KDE
    draw read the operand from the arena while the proposal goes to LDS"""
    _set_form(monkeypatch, form)
    _check(fc.below_case(cnt), 1, refs, hip_backend)


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("F", [1, 2])
def test_lazy_bandwidth_skips_the_fit_of_overwritten_outputs(F, form, refs, hip_backend, monkeypatch):
    """two fused pairs, the second overwriting the outputs of the first, under lazy_bandwidth: the first outputs' fit (for
    F = 1 the proposal's fit) is not made -- fewer likelihood evaluations than the eager program -- and the final beliefs
    are the oracle's"""
    _set_form(monkeypatch, form)
    case = fc.lazy_case(F)
    got = _check(case, 2, refs, hip_backend)
    eager = case.run(hip_backend, lazy=False)
    assert eager["nf"] == 2
    _same(case, eager, got, "the lazy program", lazy=True)
    assert got["diag"]["lcv_evals"] < eager["diag"]["lcv_evals"]


@pytest.mark.parametrize("form", ["p2", "p1"])
def test_several_write_back_flags_in_one_launch(form, refs, hip_backend, monkeypatch):
    """F = 4; a STAGE_COPIES behind the round reads inputs 0, 2 and 3 of three different updates, the last of the launch
    among them, and every proposal slot is overwritten afterwards, so that the launch carries exactly those three
    write-back flags: the copies equal the three-launch form's and the oracle's"""
    _set_form(monkeypatch, form)
    case = fc.copies_case()
    got = _check(case, 1, refs, hip_backend)
    for pts, bw, _ in got["out"][case.nops:]:
        assert np.abs(pts).max() > 0 and (bw > 0).all()
