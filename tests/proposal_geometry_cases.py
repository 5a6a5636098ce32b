"""The GPU cases of tests/test_gpu_proposal_geometries.py: every kernel a proposal launch can run (proposal_plan in csrc/nbp_api.hip:
the five workgroup instances, the three one-wave-per-proposal kernels, the two-waves-per-proposal kernel), at the sizes at which
each can still go wrong, with the kernel and the geometry the planner gives for each case (abi.plan_proposals: no context, no GPU).
tests/test_proposal_geometry_cases.py checks the list on the CPU: it reaches every (kernel, geometry) the planner can return, and
every case takes the branches it is there for on the oracle.

Sizes.  Lane l of a wave owns the particles l, l + 64, ...; measurements rotate through NC register chunks (NC = 4 up to N = 256, 5
up to 320), sums are taken chunk by chunk: N on either side of every chunk boundary, one below the last, and one N < 64.  A
workgroup of the wave kernels holds NBP_PW_WAVES = 4 proposals: sub-batches of a lone wave, a last block of three, an exact block,
a block plus one.  The split kernel's grid is the batch: one and two.

The rider batch (rider_batch) is one function for Euclid(2) and Euclid(3); every descriptor in it is "simple" as
proposals_uniform_class defines it, so the same batch runs the workgroup, the wave or the split kernel by the option set alone."""
import functools

import numpy as np

import launch_plan_cases as lpc
from parity_utils import abi, rand_points, relative_factor_desc

OPTION_SETS = {
    "defaults": {},
    "wave1": {"NBP_PROPOSAL_WAVE_MIN": "1"},
    "split1": {"NBP_PROPOSAL_SPLIT_MIN": "1"},
}
GEOMETRY = {"workgroup": 0, "wave": 1, "split": 2}
LAUNCHES = {0: (1, 0, 0), 1: (0, 1, 0), 2: (0, 0, 1)}  # proposal_launches_workgroup / _wave / _split of a case's one launch

NS_NC4 = (37, 64, 65, 128, 129, 192, 193, 255, 256)
NS_NC5 = (257, 300, 319, 320)
NS_WORKGROUP = (65, 257)
WAVE_SUB = (1, 3, 4, 5)
SPLIT_SUB = (1, 2)
# the sub-batches, by descriptor name: the waves of one workgroup run descriptors of different kinds side by side
SUB_ORDER = ("rel_solve_b", "pass_keep2", "msg_short", "rel_mixture", "rel_short_target")

FIRST_OUT = 10       # slots 0 .. 9: the beliefs the batch reads; outputs from here on
SIDE_SENTINEL = -7   # what the side memory holds before the launch
MEAN, SIG = [1.0, -0.5, 0.25], [0.1, 0.2, 0.15]


def short_count(N):
    return max(2, N - 37)


def _with(d, **fields):
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _mixture(mean, sig):
    """a two-component measurement as fuzz_proposals.make_case builds it"""
    return dict(ncomp=2, comps=[(0.7, mean, sig), (0.3, [m + 1.0 for m in mean], [s * 3 for s in sig])])


@functools.lru_cache(maxsize=None)
def rider_batch(man, N):
    """-> (writes, descs, names): the beliefs [(slot, manifold, points)] (written with belief_write and a fixed bandwidth), the
    descriptors, and their names.  Slots 0, 1, 2, 4: N points; 3: short_count(N) points; 5: a full density; 6: exactly 64 points
    (N > 64: a count that ends on a chunk boundary)."""
    D = abi.MANIFOLD_DIM[man]
    rng = np.random.default_rng(5)
    counts = {0: N, 1: N, 2: N, 3: short_count(N), 4: N, 5: N}
    if N > 64:
        counts[6] = 64
    writes = [(j, man, rand_points(rng, man, c, 1.5 * j, 0.4)) for j, c in counts.items()]
    mean, sig = MEAN[:D], SIG[:D]
    rel = lambda sf, slots, **kw: relative_factor_desc(abi.F_LINREL, man, 2, sf, slots, 0, 0, mean, sig, **kw)  # noqa: E731
    one = lambda kind, slots, **kw: relative_factor_desc(kind, man, 1, 0, slots, 0, 0, mean if kind == abi.F_PRIOR else [0], sig if kind == abi.F_PRIOR else [0], **kw)  # noqa: E731
    batch = [
        ("rel_solve_b", rel(1, [0, 1], mhidx_out=0)),                         # solve the second variable (three cycles, inflation 5)
        ("rel_solve_a", rel(0, [2, 4])),                                      # solve the first
        ("rel_short_operand", rel(1, [3, 2])),                                # an operand read through _getindex_anyn
        ("rel_short_target", rel(0, [3, 1], cycles=2)),                       # a target copy resized to N
        ("rel_one_cycle", rel(1, [0, 2], cycles=1, inflation=1.0)),
        ("rel_inflation20", rel(0, [1, 4], cycles=3, inflation=20.0)),
        ("rel_mixture", rel(1, [4, 0], mhidx_out=N, **_mixture(mean, sig))),
        ("prior", one(abi.F_PRIOR, [0])),
        ("prior_mixture", one(abi.F_PRIOR, [1], **_mixture(mean, sig))),
        ("msg_full", one(abi.F_MSGPRIOR, [0, 1])),
        ("msg_short", one(abi.F_MSGPRIOR, [2, 3])),
        ("pass_full", one(abi.F_PASSTHROUGH, [1, 5])),
        ("pass_keep0", one(abi.F_PASSTHROUGH, [1, 3])),                       # resampled to N
        ("pass_keep1", _with(one(abi.F_PASSTHROUGH, [2, 3]), keep_count=1)),  # the density's own count
        ("pass_keep2", _with(one(abi.F_PASSTHROUGH, [4, 3]), keep_count=2)),  # topped up to N from its KDE
    ]
    if N > 64:
        batch += [
            ("rel_operand64", rel(1, [6, 2])),
            ("rel_target64", rel(0, [6, 1])),
            ("pass_keep2_64", _with(one(abi.F_PASSTHROUGH, [0, 6]), keep_count=2)),
        ]
    for i, (_, d) in enumerate(batch):
        d.out_slot, d.seed = FIRST_OUT + i, 11 + i
    assert sum(d.mhidx_out >= 0 for _, d in batch) == 2
    return writes, [d for _, d in batch], [name for name, _ in batch]


OWN = {"circ": (abi.F_CIRCULAR, abi.CIRCULAR), "se2": (abi.F_SE2, abi.SE2), "generic": (abi.F_LINREL, abi.EUCLID1)}


@functools.lru_cache(maxsize=None)
def own_batch(what, N):
    """the batch of an instance without wave kernels -- CircularCircular on the circle, ManifoldFactor on SE(2), LinearRelative on
    Euclid(1) (no class: the generic kernel): two relatives, a prior, a message prior"""
    kind, man = OWN[what]
    rng = np.random.default_rng(6)
    writes = [(j, man, rand_points(rng, man, N if j != 3 else short_count(N), 0.7 * j, 0.4)) for j in range(4)]
    zd = 3 if kind == abi.F_SE2 else 1
    mean, sig = ([1.0, -0.5, 0.25][:zd], [0.1, 0.2, 0.15][:zd])
    pm, ps = MEAN[:abi.MANIFOLD_DIM[man]], SIG[:abi.MANIFOLD_DIM[man]]
    batch = [
        ("rel_solve_b", relative_factor_desc(kind, man, 2, 1, [0, 1], 0, 0, mean, sig, mhidx_out=0)),
        ("rel_solve_a", relative_factor_desc(kind, man, 2, 0, [2, 3], 0, 0, mean, sig, cycles=2, mhidx_out=N)),  # a short operand
        ("prior", relative_factor_desc(abi.F_PRIOR, man, 1, 0, [0], 0, 0, pm, ps)),
        ("msg_short", relative_factor_desc(abi.F_MSGPRIOR, man, 1, 0, [1, 3], 0, 0, [0], [0])),
    ]
    for i, (_, d) in enumerate(batch):
        d.out_slot, d.seed = FIRST_OUT + i, 31 + i
    return writes, [d for _, d in batch], [name for name, _ in batch]


def case_batch(case):
    """(writes, descs, names) of a case: its batch, or the sub-batch it picks"""
    writes, descs, names = rider_batch(case["man"], case["N"]) if case["batch"] == "rider" else own_batch(case["batch"], case["N"])
    if case["pick"] is not None:
        descs = [descs[names.index(p)] for p in case["pick"]]
        names = list(case["pick"])
    return writes, descs, names


N_SLOTS = FIRST_OUT + 20
BANDWIDTH = 0.3


def run_case(make, case):
    """the case's one launch on the backend `make(N, n_slots, side_ints)` gives -> {"rows": the raw rows of every output slot (read as
    Euclid(3): all three), "bw", "ipc", "count": per output, "side": the whole side memory, "diag": the counters of the launch}.
    The side memory holds SIDE_SENTINEL before the launch, in a third stretch of N no descriptor names as well."""
    N = case["N"]
    writes, descs, _ = case_batch(case)
    be = make(N, N_SLOTS, 3 * N)
    try:
        for slot, man, pts in writes:
            be.belief_write(slot, man, pts, np.full(abi.MANIFOLD_DIM[man], BANDWIDTH))
        be.side_write(0, np.full(3 * N, SIDE_SENTINEL, dtype=np.int32))
        be.diag(reset=True)
        be.run_proposals(descs)
        dg = be.diag()
        res = {"rows": [], "bw": [], "ipc": [], "count": [], "side": np.array(be.side_read(0, 3 * N)), "diag": dg}
        for d in descs:
            rows, bw = be.slot_read(d.out_slot, abi.EUCLID3)
            pts, _, ipc = be.belief_read(d.out_slot, abi.EUCLID3)
            res["rows"].append(rows); res["bw"].append(np.asarray(bw)); res["ipc"].append(np.asarray(ipc)); res["count"].append(pts.shape[0])
        return res
    finally:
        be.close()


@functools.lru_cache(maxsize=None)
def oracle_result(batch, man, N, pick):
    """the oracle's leg of the cases that run this batch (wave, split and workgroup cases share it); read, never changed"""
    from oracle.oracle_backend import OracleBackend
    return run_case(lambda n, s, side: OracleBackend(n, s, side, threads=8), {"batch": batch, "man": man, "N": N, "pick": pick})


def oracle_of(case):
    return oracle_result(case["batch"], case["man"], case["N"], case["pick"])


def _shapes():
    """(id, option set, batch, manifold, N, pick, the geometry the case is there for)"""
    out = []
    e2, e3 = abi.EUCLID2, abi.EUCLID3
    for N in NS_NC4:
        out += [(f"wave_lin2_N{N}", "wave1", "rider", e2, N, None, "wave"), (f"wave_lin3_N{N}", "wave1", "rider", e3, N, None, "wave"),
                (f"split_lin2_N{N}", "split1", "rider", e2, N, None, "split")]
    for N in NS_NC5:
        out.append((f"wave_lin3n5_N{N}", "wave1", "rider", e3, N, None, "wave"))
    for n in WAVE_SUB:
        pick = SUB_ORDER[:n]
        out += [(f"wave_lin2_N129_n{n}", "wave1", "rider", e2, 129, pick, "wave"), (f"wave_lin3_N129_n{n}", "wave1", "rider", e3, 129, pick, "wave"),
                (f"wave_lin3n5_N300_n{n}", "wave1", "rider", e3, 300, pick, "wave")]
    for n in SPLIT_SUB:
        out.append((f"split_lin2_N129_n{n}", "split1", "rider", e2, 129, SUB_ORDER[:n], "split"))
    for N in NS_WORKGROUP:
        out += [(f"workgroup_lin2_N{N}", "defaults", "rider", e2, N, None, "workgroup"), (f"workgroup_lin3_N{N}", "defaults", "rider", e3, N, None, "workgroup")]
        out += [(f"workgroup_{what}_N{N}", "defaults", what, OWN[what][1], N, None, "workgroup") for what in OWN]
    # refusals: beyond the rows of four / five waves the batch runs the workgroup kernel, and still equals the oracle
    out += [("refused_wave_lin2_N257", "wave1", "rider", e2, 257, None, "workgroup"), ("refused_split_lin2_N257", "split1", "rider", e2, 257, None, "workgroup"),
            ("refused_wave_lin3_N321", "wave1", "rider", e3, 321, None, "workgroup")]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for cid, oname, batch, man, N, pick, want in _shapes():
        case = {"id": cid, "options": oname, "batch": batch, "man": man, "N": N, "pick": pick, "want": want}
        n = len(case_batch(case)[1])
        with lpc.options(OPTION_SETS[oname]):
            r = abi.plan_proposals([(N, n, man, 1)])[0]
        case.update(n=n, kernel=r.kernel.decode(), geometry=r.geometry, plan=r.as_dict())
        out.append(case)
    return out
