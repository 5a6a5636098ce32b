"""-m gpu: a finalized program handed new seeds (nbp_program_set_seeds; what the native host's plan cache does to a cached
level program) on rounds that run on two streams (nbp_api.hip plan_pipeline; environment NBP_PIPELINE_MIN).  Such a round has
its descriptors reordered inside their stages, the caller keeps handing its seeds over in the order of ITS stages, and a seed
in the wrong descriptor still gives a plausible posterior: only a comparison bit for bit, against the right keys, notices.

The reference of every comparison is the CPU checker (oracle/), which runs the stages one descriptor at a time in the caller's
order and knows nothing of halves, streams, graphs or caches: "the checker's run of the stages that carry seed set B" is what
set_seeds(B) must produce.  np.array_equal on the points and the bandwidth of every slot the program writes.

Every case shows from the library's own counters that it is not vacuous: num_two_stream() > 0 in the pipelined leg and 0 in the
control, the hand-made round really reordered (seed_order()), cache hits and two-stream rounds in cached programs."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from parity_utils import ROOT, abi, iif, product_desc, rand_points, relative_factor_desc

pytestmark = pytest.mark.gpu

N, NUPD = 100, 256  # 256 updates: both rounds reach NBP_PIPELINE_MIN = 128, the smallest batch the planner splits


@pytest.fixture
def pipeline_env():
    def set_(v):
        if v is None:
            os.environ.pop("NBP_PIPELINE_MIN", None)
        else:
            os.environ["NBP_PIPELINE_MIN"] = str(v)
    yield set_
    os.environ.pop("NBP_PIPELINE_MIN", None)


def _differing(want, got):
    """slots whose points or bandwidth are not the reference's bytes"""
    return sorted(k for k in want if not (np.array_equal(want[k][0], got[k][0]) and np.array_equal(want[k][1], got[k][1])))


# ---- items 1 to 3: a hand-made program of two rounds, op level --------------------------------------------------------------
# relative factor (kind, mean, sigma) and the prior's sigma per manifold
_FACTORS = {abi.EUCLID2: (abi.F_LINREL, [1.0, 0.5], [0.1, 0.1], [0.3, 0.3]),
            abi.SE2: (abi.F_SE2, [1.0, 0.2, 0.3], [0.1, 0.1, 0.01], [0.3, 0.3, 0.1])}


def _belief(i):
    return 2 + i


def _proposal_slots(r, i):
    a = 2 + NUPD + 4 * i + 2 * r
    return a, a + 1


_DECONV0 = 2 + 5 * NUPD
_NSLOTS = _DECONV0 + NUPD // 4


def _hand_made(man, variant, base, step):
    """[(PROPOSALS, props), (PRODUCTS, prods)] x 2 over NUPD beliefs, every descriptor with a seed of its own (base + step * its
    place in the caller's order).  The updates are coupled in pairs (update i's relative proposal reads the belief update i ^ 1
    writes), so the planner keeps a pair in one half and sends the pairs -- components of equal weight -- to alternating halves:
    caller order and program order differ for most descriptors.
    variant "stored": a share of the proposals reuses the measurement another proposal drew (meas_seed names that one's seed),
    in between proposals that carry none.  variant "deconv": a DECONV stage in front.
    -> (stages, [(slot, manifold) the program writes], [(i, j): prior i reuses the measurement of the fresh prior j, per round])"""
    kind, rel_mu, rel_sig, pri_sig = _FACTORS[man]
    D = abi.MANIFOLD_DIM[man]
    count = itertools.count()

    def seed():
        return base + step * next(count)

    stages, written, reuse = [], [], []
    if variant == "deconv":
        zman = {2: abi.EUCLID2, 3: abi.EUCLID3}[D]
        decs = [relative_factor_desc(kind, man, 2, 1, [_belief(i), _belief(i ^ 1)], _DECONV0 + j, seed(), [0.0] * D, [1.0] * D)
                for j, i in enumerate(range(0, NUPD, 4))]
        stages.append((abi.STAGE_DECONV, decs))
        written += [(d.out_slot, zman) for d in decs]
    for r in range(2):
        props, prods = [], []
        for i in range(NUPD):
            a, b = _proposal_slots(r, i)
            props.append(relative_factor_desc(kind, man, 2, 1, [_belief(i ^ 1), _belief(i)], a, seed(), rel_mu, rel_sig))
            props.append(relative_factor_desc(abi.F_PRIOR, man, 1, 0, [_belief(i)], b, seed(), [float(i % 8)] + [0.0] * (D - 1), pri_sig))
            prods.append(product_desc(man, [a, b], _belief(i), seed()))
            written += [(a, man), (b, man)]
        if variant == "stored":
            for i in range(NUPD):
                j = (i + 8) % NUPD  # a prior with the same mean: the same measurement gives the same points
                if i % 3 == 0:
                    props[2 * i + 1].meas_seed = props[2 * j + 1].seed
                    if j % 3 and r == 1:
                        reuse.append((i, j))
                if i % 5 == 1:
                    props[2 * i].meas_seed = props[2 * (i ^ 1)].seed
        stages += [(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)]
    written += [(_belief(i), man) for i in range(NUPD)]
    return stages, written, reuse


def _start(man):
    return [(_belief(i), rand_points(np.random.default_rng(100 + i), man, N, float(i % 8), 0.5)) for i in range(NUPD)]


def _run_hip(man, stages, written, runs, seeds_then=None):
    """the program run `runs` times from the same beliefs; the last run with `seeds_then` (the second run of a range is
    captured, the third a hipGraph replay -- with the fork and the join of a two-stream round inside)"""
    be = iif.HipBackend(N, _NSLOTS, 0)
    try:
        prog = be.program(stages, lazy_bandwidth=True)
        n2 = prog.num_two_stream()
        for r in range(runs):
            for s, pts in _start(man):
                be.slot_write(s, man, pts)
            if seeds_then is not None and r == runs - 1:
                prog.set_seeds(seeds_then)
            prog.run()
            be.synchronize()
        out = {s: be.slot_read(s, m) for s, m in written}
        prog.close()
        return n2, out
    finally:
        be.close()


def _run_oracle(oracle_backend, man, stages, written):
    be = oracle_backend(N, _NSLOTS, 0)
    for s, pts in _start(man):
        be.slot_write(s, man, pts)
    be.program(stages).run()
    return {s: be.slot_read(s, m) for s, m in written}


def _seed_order(stages):
    be = iif.HipBackend(N, _NSLOTS, 0)
    try:
        prog = be.program(stages, lazy_bandwidth=True)
        order = prog.seed_order()
        prog.close()
        return order
    finally:
        be.close()


@pytest.mark.parametrize("man,variant,runs", [
    (abi.EUCLID2, "plain", 1), (abi.EUCLID2, "plain", 3), (abi.SE2, "plain", 1), (abi.SE2, "plain", 3),
    (abi.EUCLID2, "stored", 3), (abi.SE2, "stored", 1), (abi.EUCLID2, "deconv", 3),
], ids=["euclid2-plain-1", "euclid2-plain-3", "se2-plain-1", "se2-plain-3", "euclid2-stored-3", "se2-stored-1", "euclid2-deconv-3"])
def test_reseeded_two_stream_round_is_the_checkers_run_of_the_new_seeds(oracle_backend, pipeline_env, man, variant, runs):
    """compiled with seed set A, handed set B (set_seeds), run: the checker's run of the stages carrying B, and the library's own
    run of the program compiled with B -- with the rounds on two streams (NBP_PIPELINE_MIN = 128) and, the control, on one.
    (Before the seed table followed the caller's order, set_seeds gave descriptor k of a two-stream round the seed meant for the
    descriptor the planner had put in its place: the pipelined leg differs, the control does not.)"""
    from iif_amd.backend import HipProgram
    sa, wr, _ = _hand_made(man, variant, 1000, 1)
    sb, _, reuse = _hand_made(man, variant, 7000000, 3)
    seeds_a, seeds_b = HipProgram.seeds_of(sa), HipProgram.seeds_of(sb)
    own = [d.seed for stages in (sa, sb) for _, ds in stages for d in ds]
    assert len(seeds_a) == len(seeds_b) and len(set(own)) == len(own) >= 2 * (6 * NUPD)  # every descriptor a seed of its own, in A and in B
    if variant == "stored":  # seeds and stored measurements interleave in the list: a wrong order moves values between the two fields
        n_meas = sum(1 for k, ds in sb if k == abi.STAGE_PROPOSALS for d in ds if d.meas_seed)
        assert n_meas > NUPD // 2 and len(seeds_b) == 2 * (3 * NUPD) + n_meas and reuse
    want = _run_oracle(oracle_backend, man, sb, wr)
    res = {}
    for pipe in (None, 128):
        pipeline_env(pipe)
        n2, got = _run_hip(man, sa, wr, runs, seeds_then=seeds_b)
        n2b, direct = _run_hip(man, sb, wr, 1)
        res[pipe] = (n2, n2b, _differing(want, got), _differing(want, direct), got)
        print(f"[reseeded op level] {variant} manifold {man} runs {runs} NBP_PIPELINE_MIN {pipe}: two-stream rounds {n2}; "
              f"slots differing from the checker on B: {len(res[pipe][2])} of {len(want)} after set_seeds(B), {len(res[pipe][3])} compiled with B")
    for pipe, (n2, n2b, bad, bad_direct, got) in res.items():
        assert n2 == n2b == (2 if pipe else 0), (pipe, n2, n2b)
        assert not bad_direct, (pipe, len(bad_direct), bad_direct[:8])
        assert not bad, (pipe, len(bad), bad[:8])
        # the reused measurement is the one the named op drew: a prior's proposal IS its measurement (round 2's slots)
        for i, j in reuse:
            assert np.array_equal(got[_proposal_slots(1, i)[1]][0], got[_proposal_slots(1, j)[1]][0]), (pipe, i, j)
    # the hand-made round really is reordered: most seeds go to another place than the caller's, and only in the pipelined leg
    pipeline_env(None)
    assert _seed_order(sa) == list(range(len(seeds_a)))
    pipeline_env(128)
    order = _seed_order(sa)
    assert sorted(order) == list(range(len(seeds_a)))
    moved = sum(1 for i, o in enumerate(order) if i != o)
    print(f"[reseeded op level] {variant}: {moved} of {len(order)} seeds go to another place than the caller's")
    assert moved > len(order) // 2, moved


# ---- item 4: tree programs with two-stream rounds --------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["chain", "lattice"])
def test_reseeded_tree_program_with_two_stream_rounds(oracle_backend, hip_backend, pipeline_env, build):
    """test_gpu_properties.py::test_program_with_new_seeds_is_the_program_compiled_with_them on graphs whose tree programs split
    (the ones of test_gpu_pipelined_rounds.py), against the checker's run of the tree program compiled with the new seed"""
    from iif_amd.backend import HipProgram
    fg = {"chain": lambda: iif.generateChainEuclid(600, vardims=2, priorEvery=50, N=N),
          "lattice": lambda: iif.generateSE2Lattice(rows=20, cols=40, N=N, closeEvery=2)}[build]()
    iif.initAll(fg, backend=hip_backend, seed=3)
    tree = iif.buildTreeReset(fg, iif.nestedDissectionOrder(fg))
    tpa, tpb = iif.TreeProgram(fg, tree, seed=11), iif.TreeProgram(fg, tree, seed=12)
    sa, sb = HipProgram.seeds_of(tpa.stages), HipProgram.seeds_of(tpb.stages)
    assert len(sa) == len(sb) and sa != sb

    def solve(be, tp, seeds_then=None, runs=1):
        prog = be.program(tp.stages, lazy_bandwidth=True)
        n2 = prog.num_two_stream() if seeds_then is not None else None
        for r in range(runs):
            for v in fg.ls():
                var = fg.getVariable(v)
                be.belief_write(tp.main[v], var.varType.manifold, var.val, var.bw)
            iif.solver.write_densities(fg, be)
            if seeds_then is not None and r == runs - 1:
                prog.set_seeds(seeds_then)
            prog.run()
            be.synchronize()
        out = {v: be.slot_read(tp.main[v], fg.getVariable(v).varType.manifold) for v in fg.ls()}
        prog.close()
        be.close()
        return n2, out

    _, want = solve(oracle_backend(N, tpb.n_slots), tpb)
    res = []
    for pipe in (None, 128):
        pipeline_env(pipe)
        for runs in (1, 3):  # (3: the re-seeded run is a hipGraph replay)
            n2, got = solve(hip_backend(N, tpa.n_slots), tpa, seeds_then=sb, runs=runs)
            res.append((pipe, runs, n2, _differing(want, got)))
            print(f"[reseeded tree] {build} NBP_PIPELINE_MIN {pipe} runs {runs}: two-stream rounds {n2}; "
                  f"posteriors differing from the checker on seed 12: {len(res[-1][3])} of {len(want)}")
    for pipe, runs, n2, bad in res:
        assert (n2 > 0) if pipe else (n2 == 0), (pipe, n2)
        assert not bad, (pipe, runs, len(bad), bad[:8])


# ---- item 5: the native host's plan cache on a two-stream level -------------------------------------------------------------
_STATS = re.compile(r"plan cache: (\d+) hits, (\d+) misses, (\d+) programs kept, (\d+) two-stream rounds in cached programs")
_NVARS, _WALKS = 600, 6


@pytest.mark.parametrize("mode", ["0", "-1"], ids=["solve_batch", "submit_batch"])
def test_plan_cache_reseeds_levels_with_two_stream_rounds(tmp_path, mode):
    """examples/solve_by_clique_calls.c, one batch per tree level (nbp_clique_solve_batch / nbp_clique_submit_batch), six walks of a
    600-variable chain with a seed of their own each and the whole-tree program's seed on the last: from the second walk on every
    level is a cached program handed new seeds.  With NBP_PIPELINE_MIN = 128 the wide levels are two-stream rounds.  Every walk's
    posteriors must be the bytes of the same walk without the cache, and the last walk's the whole-tree program's (the example's
    own comparison; that program equals the checker's run, test_gpu_stagewise_parity.py / test_gpu_pipelined_rounds.py)."""
    lib = os.path.join(ROOT, "incrementalinference.jl_amd", "csrc")
    exe = str(tmp_path / "clique_calls")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-fopenmp", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "solve_by_clique_calls.c"),
                           "-o", exe, "-L", lib, "-lnbp", f"-Wl,-rpath,{lib}", "-lm"])

    def walks(name, **extra):
        env = {k: v for k, v in os.environ.items() if k not in ("NBP_PIPELINE_MIN", "NBP_PLAN_CACHE", "NBP_PLAN_CACHE_ENTRIES")}
        env.update(NBP_WALKS=str(_WALKS), NBP_WALK_SEEDS="1", NBP_PLAN_CACHE_STATS="1", NBP_WALK_DUMP=str(tmp_path / name), **extra)
        out = subprocess.run([exe, str(_NVARS), str(N), "20", mode], capture_output=True, text=True, timeout=600, env=env)
        stats = [sum(int(m[k]) for m in _STATS.findall(out.stderr)) for k in range(4)] if _STATS.search(out.stderr) else None
        dump = np.fromfile(str(tmp_path / name)) if os.path.exists(str(tmp_path / name)) else np.zeros(0)
        return out, stats, dump

    cached, st, d_cached = walks("cached", NBP_PIPELINE_MIN="128")
    plain, st_plain, d_plain = walks("plain", NBP_PIPELINE_MIN="128", NBP_PLAN_CACHE="0")
    control, st_control, _ = walks("control")
    per_walk = _NVARS * (2 * N + 2)
    assert d_plain.size == d_cached.size == _WALKS * per_walk, (d_plain.size, d_cached.size, cached.stdout + cached.stderr, plain.stdout + plain.stderr)
    a, b = d_cached.view(np.uint64).reshape(_WALKS, _NVARS, -1), d_plain.view(np.uint64).reshape(_WALKS, _NVARS, -1)
    bad = [int((a[w] != b[w]).any(axis=1).sum()) for w in range(_WALKS)]
    print(f"[reseeded plan cache] mode {mode}: plan cache (hits, misses, kept, two-stream rounds in cached programs) = {st}, control {st_control}; "
          f"posteriors per walk that are not the bytes of the walk without the cache: {bad} of {_NVARS}; last walk: {cached.stdout.splitlines()[:1]}")
    # not vacuous: the cache was hit, and programs it re-seeded hold two-stream rounds -- none in the control
    assert st is not None and st[0] > 0 and st[3] > 0, (st, cached.stderr[-500:])
    assert st_plain is None, plain.stderr[-500:]  # (no cache, no statistics)
    assert st_control is not None and st_control[0] > 0 and st_control[3] == 0, st_control
    assert bad == [0] * _WALKS, bad
    for out in (plain, cached, control):
        assert f"{_NVARS} of {_NVARS} posteriors byte-identical" in out.stdout, out.stdout + out.stderr[-500:]
        assert out.returncode == 0, out.stdout + out.stderr
