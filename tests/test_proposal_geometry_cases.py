"""CPU: the case list of tests/test_gpu_proposal_geometries.py (tests/proposal_geometry_cases.py).

Coverage is asserted, not claimed: the plan query of the library (nbp_plan_proposals: proposal_plan itself, no GPU) is swept over
every particle count a context can have, the batch sizes on either side of every threshold, every manifold class and none, simple
or not, under the three option sets of the cases; the (kernel, geometry) pairs it can return are exactly those the case list
reaches.  A threshold that moves, or a tenth kernel, fails here instead of silently losing its comparison with the oracle.

And every case runs on the oracle alone: everything finite, and the branches the case is there for really taken."""
import numpy as np
import pytest

import launch_plan_cases as lpc
import proposal_geometry_cases as pgc
from parity_utils import abi

SWEEP_N = range(8, 513)  # (a context, and so a plan, has 8 .. 512 particles: below that the query refuses, see the test)
SWEEP_n = (1, 2, 3, 4, 5, 599, 600, 1499, 1500, 3499, 3500, 10000)
WORKGROUP = {"nbp_proposal_kernel", "nbp_proposal_kernel_lin2", "nbp_proposal_kernel_lin3", "nbp_proposal_kernel_circ", "nbp_proposal_kernel_se2"}
WAVE = {"nbp_proposal_wave_kernel_lin2", "nbp_proposal_wave_kernel_lin3", "nbp_proposal_wave_kernel_lin3n5"}
SPLIT = {"nbp_proposal_split_kernel_lin2"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return abi.load_library()


@pytest.fixture(scope="module")
def reachable(lib):
    """every (kernel, geometry) the planner returns over the sweep"""
    reqs = [(N, n, m, simple) for N in SWEEP_N for n in SWEEP_n for m in range(0, abi.SE2 + 1) for simple in (0, 1)]
    out = set()
    for env in pgc.OPTION_SETS.values():
        with lpc.options(env):
            recs = abi.plan_proposals(reqs)
        for r in recs:
            assert r.status == 0
            out.add((r.kernel.decode(), r.geometry))
    return out


def test_the_case_list_reaches_every_kernel_the_planner_can_return(reachable):
    cases = pgc.cases()
    assert len({c["id"] for c in cases}) == len(cases)
    reached = {(c["kernel"], c["geometry"]) for c in cases}
    assert reached == reachable, (reachable - reached, reached - reachable)
    assert reachable == {(k, 0) for k in WORKGROUP} | {(k, 1) for k in WAVE} | {(k, 2) for k in SPLIT}  # nine kernels today
    print(f"{len(cases)} proposal geometry cases, {len(reachable)} kernels")


def test_no_plan_below_eight_particles(lib):
    """the issue's sweep starts at N = 2: no context has fewer than 8 particles, and the query says so instead of planning"""
    for N in range(2, 8):
        with pytest.raises(ValueError):
            abi.plan_proposals([(N, 1, abi.EUCLID2, 1)])


def test_every_case_is_planned_onto_the_kernel_it_is_there_for(lib):
    cases = {c["id"]: c for c in pgc.cases()}
    for c in cases.values():
        assert c["geometry"] == pgc.GEOMETRY[c["want"]], c
        kind = c["id"].split("_N")[0]
        if c["want"] == "workgroup":  # (the refusals: the workgroup instance of the class)
            suffix = {abi.EUCLID2: "_lin2", abi.EUCLID3: "_lin3", abi.CIRCULAR: "_circ", abi.SE2: "_se2", abi.EUCLID1: ""}[c["man"]]
            assert c["kernel"] == "nbp_proposal_kernel" + suffix, c
        else:
            assert c["kernel"] == f"nbp_proposal_{c['want']}_kernel_{kind.split('_')[1]}", c
    # the sizes: every chunk boundary of the wave and split kernels, the sub-batches, both sizes of every workgroup instance
    for N in pgc.NS_NC4:
        assert {f"wave_lin2_N{N}", f"wave_lin3_N{N}", f"split_lin2_N{N}"} <= set(cases)
        assert cases[f"wave_lin2_N{N}"]["n"] == len(pgc.rider_batch(abi.EUCLID2, N)[1])
    for N in pgc.NS_NC5:
        assert f"wave_lin3n5_N{N}" in cases
    for n in pgc.WAVE_SUB:
        for k, N in (("lin2", 129), ("lin3", 129), ("lin3n5", 300)):
            assert cases[f"wave_{k}_N{N}_n{n}"]["n"] == n and cases[f"wave_{k}_N{N}_n{n}"]["plan"]["blocks"] == (n + 3) // 4
    for n in pgc.SPLIT_SUB:
        assert cases[f"split_lin2_N129_n{n}"]["n"] == n
    for N in pgc.NS_WORKGROUP:
        assert {c["kernel"] for c in cases.values() if c["N"] == N and c["options"] == "defaults"} == WORKGROUP


def test_every_descriptor_of_the_rider_batch_is_simple():
    for man in (abi.EUCLID2, abi.EUCLID3):
        for N in (37, 129):
            _, descs, names = pgc.rider_batch(man, N)
            assert len(set(names)) == len(names) and len({d.out_slot for d in descs}) == len(descs)
            for d in descs:
                assert d.manifold == man and not d.partial_mask and not d.has_multihypo and d.nullhypo == 0.0 and d.mhidx_in < 0
                assert d.factor_kind in (abi.F_PRIOR, abi.F_MSGPRIOR, abi.F_PASSTHROUGH) or (d.factor_kind == abi.F_LINREL and d.nvars == 2)
                assert max(d.out_slot, *[d.var_slot[k] for k in range(2)]) < pgc.N_SLOTS
            assert sorted(d.mhidx_out for d in descs if d.mhidx_out >= 0) == [0, N]
            assert {d.inflate_cycles for d in descs if d.factor_kind == abi.F_LINREL} >= {1, 2, 3}
            assert {d.keep_count for d in descs if d.factor_kind == abi.F_PASSTHROUGH} == {0, 1, 2}
            assert ("rel_operand64" in names) == (N > 64)


def _rows_of(writes, slot, D):
    return next(pts for s, _, pts in writes if s == slot)[:, :D]


@pytest.mark.parametrize("case", pgc.cases(), ids=lambda c: c["id"])
def test_the_case_takes_its_branches_on_the_oracle(case):
    N, man = case["N"], case["man"]
    D = abi.MANIFOLD_DIM[man]
    writes, descs, names = pgc.case_batch(case)
    res = pgc.oracle_of(case)
    for name, rows, bw, count in zip(names, res["rows"], res["bw"], res["count"]):
        assert np.isfinite(rows).all() and np.isfinite(bw).all(), name
        assert count == (pgc.short_count(N) if name == "pass_keep1" else N), name
    assert res["diag"]["solves"] > 0 or not any(n.startswith("rel") for n in names)
    side = res["side"]
    named = np.zeros(3 * N, dtype=bool)
    for d in descs:
        if d.mhidx_out >= 0:
            named[d.mhidx_out:d.mhidx_out + N] = True
    assert (side[named] == 1).all() and (side[~named] == pgc.SIDE_SENTINEL).all()
    if case["batch"] != "rider":
        return
    by = dict(zip(names, zip(descs, res["rows"])))
    for name, (d, rows) in by.items():
        if d.factor_kind != abi.F_PASSTHROUGH:
            continue
        den = _rows_of(writes, d.var_slot[1], D)
        cd = den.shape[0]
        if name == "pass_full":
            assert cd == N and np.array_equal(rows[:, :D], den)
            continue
        assert cd < N
        if d.keep_count == 1:    # the density's points, as many as it has
            assert np.array_equal(rows[:cd, :D], den)
        elif d.keep_count == 2:  # the density's own points first, then draws from its KDE: none of them one of its points
            assert np.array_equal(rows[:cd, :D], den)
            assert not (rows[cd:, None, :D] == den[None, :, :]).all(axis=2).any()
            assert (np.abs(rows[cd:, None, :D] - den[None, :, :]).max(axis=2).min(axis=1) < 6 * pgc.BANDWIDTH).all()
        else:                    # N draws among cd < N points: every one a point of the density, some point drawn twice
            hit = (rows[:, None, :D] == den[None, :, :]).all(axis=2)
            assert hit.any(axis=1).all() and hit.sum(axis=0).max() > 1
    for name in ("rel_mixture", "prior_mixture"):
        if name not in by:
            continue
        d, rows = by[name]
        # coordinate 0 of the measurement: component 0 at MEAN[0] +- 0.1 (weight 0.7), component 1 at MEAN[0] + 1 +- 0.3
        z0 = rows[:, 0] - (_rows_of(writes, d.var_slot[0], D)[:, 0] if name == "rel_mixture" else 0.0) - pgc.MEAN[0]
        first, second = int((np.abs(z0) < 0.45).sum()), int((z0 > 0.45).sum())
        assert first > N // 3 and second > N // 10 and first + second == N, (name, first, second)
