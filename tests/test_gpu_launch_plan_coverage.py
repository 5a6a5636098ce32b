"""-m gpu: the smallest launch of every distinct launch plan, held to the oracle.

What a product or fit launch runs is decided on the host (product_plan / fit_plan in csrc/nbp_api.hip); the kernel then lays out
its LDS on its own.  The cases here are computed at collection with the plan queries of the library (tests/launch_plan_cases.py:
one case per plan signature the candidate shapes reach, under the option sets of the CPU sweep of tests/test_launch_plans.py --
the switches are set while the context is created, which is when the library reads them).  Every case

  * runs its batch on the device and the first, the middle and the last product (and the two-density product of a batch whose
    largest density count is three or more) on the oracle: points and labels equal bit for bit, everything finite;
  * asserts that the plan the launch RECORDED (nbp_last_plans) is the plan the case was chosen for -- a case whose launch ran
    another kernel fails instead of passing on it.

Fits: beliefs from rand_points, bandwidths equal to the oracle's bit for bit, for the plain launches (run_bandwidth) and the prep
launches (the KD builds of one product batch; and a program's round, whose prep launch runs the fits of its proposals beside the
KD builds of its products -- the speculative prep kernels).  No tolerance anywhere."""
import numpy as np
import pytest

from fused_cases import legacy_round
from launch_plan_cases import FIT_MANIFOLD, FIT_OPTION_SETS, OPTION_SETS, fit_cases, options, product_cases, product_keep, product_specs
from parity_utils import abi, iif, rand_points
from test_gpu_latency_product_instances import run

pytestmark = pytest.mark.gpu

PLAN_FIELDS = ("status", "HL", "wpb", "G", "big", "xs", "circ", "nch", "all_levels", "w1", "row", "kernel", "launch_bound", "lds", "gstats",
               "N", "n", "F", "D", "mani", "geom_n")
FIT_FIELDS = ("P", "depth", "KS", "w5", "threads", "prep", "lds", "kernel", "N", "fits", "coords", "products", "kdF")


def _hip_under(env):
    def make(N, n_slots, side_ints=0):
        with options(env):
            return iif.HipBackend(N, n_slots, side_ints=side_ints)
    return make


@pytest.mark.parametrize("case", product_cases(), ids=lambda c: c["id"])
def test_products_of_every_plan_equal_the_oracle(case, oracle_backend):
    N, n, F = case["N"], case["n"], case["F"]
    specs = product_specs(case["kind"], n, F)
    keep = product_keep(n, F)
    if F >= 3:
        assert specs[1][1] == 2 and 1 in keep  # the launch mixes density counts, and the small product is compared
    ran = {}
    pts, labs = run(_hip_under(OPTION_SETS[case["options"]]), N, specs, plans=ran)
    want, got = case["plan"], ran["product"]
    assert {k: got[k] for k in PLAN_FIELDS} == {k: want[k] for k in PLAN_FIELDS}, "the launch did not run the plan this case was chosen for"
    assert ran["prep"]["kd_nostats"] == want["xs"], "the prep launch and the product launch disagree about the node sums (_xs)"
    opts, olabs = run(oracle_backend, N, specs, keep=keep)
    for i in range(n):
        assert np.isfinite(pts[i]).all(), f"product {i}"
    for i in keep:
        assert np.array_equal(pts[i], opts[i]), f"product {i} ({specs[i][1]} densities): points differ from the oracle's"
        assert np.array_equal(labs[i], olabs[i]), f"product {i} ({specs[i][1]} densities): labels differ from the oracle's"


def _fit_leg(make, case, ran=None):
    """-> the bandwidths the case's launch fitted: of `n` beliefs (plain), or of the first, middle and last of `n` products (prep)"""
    N, n, man = case["N"], case["n"], FIT_MANIFOLD
    rng = np.random.default_rng(3)
    if case["what"] == "plain":
        beliefs = [rand_points(rng, man, N, 0.1 * (j % 17), 0.2 + 0.01 * (j % 5)) for j in range(n)]
        keep = sorted({0, n // 2, n - 1})
        slots = list(range(n)) if ran is not None else keep  # (the oracle: the fits that are compared -- each is its own belief's)
        be = make(N, n, 0)
        try:
            for j in slots:
                be.slot_write(j, man, beliefs[j])
            be.run_bandwidth(slots, [man] * len(slots))
            if ran is not None:
                ran.update(be.last_plans())
            return [be.slot_read(j, man)[1] for j in keep]
        finally:
            be.close()
    keep = sorted({0, n // 2, n - 1})
    if case["what"] == "round":
        props, prods, stride = legacy_round(n, 2)
        be = make(N, 4 + stride * n, 0)
        try:
            for s, centre in enumerate((0.0, 2.0, 1.0)):
                be.slot_write(s, man, rand_points(rng, man, N, centre, 0.4))
            prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)])
            try:
                prog.run()
                be.synchronize()
                if ran is not None:
                    ran.update(be.last_plans())
                return [np.concatenate([x.ravel() for x in be.slot_read(4 + stride * i + 2, man)]) for i in keep]
            finally:
                prog.close()
        finally:
            be.close()
    nsrc = 4
    be = make(N, nsrc + n, 0)
    try:
        for j in range(nsrc):
            be.slot_write(j, man, rand_points(rng, man, N, 0.3 * j, 0.3))
        be.run_bandwidth(list(range(nsrc)), [man] * nsrc)
        descs = [iif.solver.product_desc(man, [i % nsrc, (i + 1) % nsrc], nsrc + i, 21 + i) for i in range(n)]
        be.run_products(descs if ran is not None else [descs[i] for i in keep])
        if ran is not None:
            ran.update(be.last_plans())
        return [np.concatenate([x.ravel() for x in be.slot_read(nsrc + i, man)]) for i in keep]
    finally:
        be.close()


@pytest.mark.parametrize("case", fit_cases(), ids=lambda c: c["id"])
def test_fits_of_every_plan_equal_the_oracle(case, oracle_backend):
    ran = {}
    got = _fit_leg(_hip_under(FIT_OPTION_SETS[case["options"]]), case, ran)
    rec = ran["fits" if case["what"] == "plain" else "prep"]
    assert {k: rec[k] for k in FIT_FIELDS} == {k: case["plan"][k] for k in FIT_FIELDS}, "the launch did not run the plan this case was chosen for"
    want = _fit_leg(oracle_backend, case)
    for g, w in zip(got, want):
        assert np.isfinite(g).all()
        assert np.array_equal(g, w), "bandwidths (prep: the product fitted behind the KD builds) differ from the oracle's"
