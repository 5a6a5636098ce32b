"""-m gpu: the product sampler leaves out the one label draw of a pass that nothing reads.

`product_body` draws, per pass, a label on the point x for the densities 1 .. F-1 only (`sampleIndices!`), then `niter` sweeps
of `sampleIndex`.  The draw on the point of density 0 is dead: a draw on the point reads no label, the first draw of the first
sweep (density 0; niter >= 1) reads the labels of the other densities and overwrites label 0, and the moments of the next
point are taken behind the sweeps.  The random streams are keyed by (sample, pass, density, purpose), so no other draw's
uniform moves.  The oracle (`oracle/`) still makes that draw; the device's points AND labels must be the oracle's, bit for bit,
for every kernel that runs `product_body`:

  * F = 2, 3, 4; every manifold; full inputs and (dimension >= 2) partial inputs -- the partial batches mix three mask
    patterns, one of which leaves coordinate 0 to the old points; niter 1 and 3;
  * every geometry `product_plan` (csrc/nbp_api.hip) can choose, by batch size: a lone product (y32), 40 (l8), 500 (t2: the
    `_xs` single-manifold instances for full inputs, the generic t2 kernel for partial ones), the same 500 with
    NBP_NO_XS_PRODUCTS (the single-manifold instances that read the node sums of the KD workspace), and 200 products at N = 512,
    where three and four densities of a manifold of dimension >= 2 do not fit the LDS (`big`: node statistics in global
    memory, generic l8 kernel; two densities never exceed the LDS at N <= 512 and run the wide t2 instances there; three partial
    densities on Euclid(2) fit as well, in the generic t2 kernel);
  * the fused update kernel under NBP_FUSED_MIN, in both of its forms (two helper rows per update, and one lane per particle
    under NBP_FUSED_P1_MIN).  It takes Euclid(2) rounds without label output only (`fused_plan`), so points and bandwidths
    are what is compared there.

The harness is the one of test_gpu_latency_product_instances.py (`run`: sources, descriptors, label areas, a fixed subset of
the batch on the oracle) and of test_gpu_fused_update.py (`_round`); `niter` goes into their descriptors on the way to the
backend.  Exact equality throughout, no case skipped, the set of cases fixed.

Every case asserts the plan its launch recorded (HipBackend.last_plans) against what its geometry stands for -- `_assert_geometry` --
so that a moved threshold fails the case instead of moving it to another kernel."""
import numpy as np
import pytest

from parity_utils import abi, rand_points
from test_gpu_fused_update import MAN as FUSED_MAN
from test_gpu_fused_update import N as FUSED_N
from test_gpu_fused_update import _round
from test_gpu_latency_product_instances import MANIS, hip, run

pytestmark = pytest.mark.gpu

# geometry -> (particles, products, environment of the context)
GEOMS = {
    "y32": (200, 1, {}),
    "l8": (200, 40, {}),
    "t2": (200, 500, {}),
    "t2_noxs": (200, 500, {"NBP_NO_XS_PRODUCTS": "1"}),
    "n512": (512, 200, {}),
}


class _WithNiter:
    """a backend whose product descriptors all carry `niter` (the imported harness writes niter = 1)"""

    def __init__(self, be, niter):
        self._be, self._niter = be, niter

    def __getattr__(self, name):
        return getattr(self._be, name)

    def run_products(self, descs):
        for d in descs:
            d.niter = self._niter
        return self._be.run_products(descs)


def _masks(D, F, i):
    """partial masks of product i: partial + full, all partial with every coordinate informed, coordinate 0 uninformed"""
    rest = (1 << D) - 2
    return ([1, 0, rest, 0], [rest, 1, 0, 1], [2, 2, 2, 2])[i % 3][:F]


def _specs(name, F, n, partial):
    man, D = MANIS[name], abi.MANIFOLD_DIM[MANIS[name]]
    return [(man, F, _masks(D, F, i) if partial else None) for i in range(n)]


def _assert_geometry(geom, name, partial, F, plan):
    """the recorded plan of the launch is the one GEOMS[geom] is there for (the docstring above)"""
    N, n, _ = GEOMS[geom]
    D = abi.MANIFOLD_DIM[MANIS[name]]
    assert (plan["status"], plan["N"], plan["n"], plan["F"], plan["geom_n"]) == (0, N, n, F, 0), plan
    generic = plan["row_mani"] == 0
    assert generic == (partial or bool(plan["big"])) and plan["mani"] == (0 if partial else MANIS[name]), plan  # partial and big: generic kernels
    if geom in ("y32", "l8"):
        assert plan["HL"] == (32 if geom == "y32" else 8) and not plan["big"] and not plan["xs"], plan
        assert plan["kernel"].startswith(f"nbp_product_kernel_{geom}" + ("" if partial else f"_{name}")), plan
    elif geom in ("t2", "t2_noxs"):
        assert plan["HL"] == 2 and not plan["big"], plan
        assert plan["xs"] == (geom == "t2" and not partial), plan  # an `_xs` row for full inputs, the KD workspace's node sums otherwise
        assert plan["kernel"] == "nbp_product_kernel_t2" + ("" if partial else f"_{name}" + ("_xs" if geom == "t2" else "")), plan
    else:  # n512: three and four densities of a manifold of dimension >= 2 do not fit the LDS ...
        # ... but for three PARTIAL densities on Euclid(2): the generic t2 kernel runs them in two workgroups of eight waves, whose
        # label table and chunk sums are half those of the one wide workgroup of the full batch, and the statistics fit (147 KB)
        assert plan["big"] == int(F >= 3 and D >= 2 and not (partial and name == "e2" and F == 3)), plan
        if plan["big"]:
            assert plan["HL"] == 8 and plan["kernel"] == "nbp_product_kernel_l8" and plan["gstats"] > 0, plan
        else:
            assert plan["HL"] == 2, plan
            if not partial and name in ("e1", "e2", "e3"):
                assert (plan["wpb"], plan["G"]) == (16, 1), plan  # the wide t2 instances: one workgroup of sixteen waves


def _cases():
    out = []
    for geom in GEOMS:
        for name in MANIS:
            for partial in (False, True):
                if partial and (abi.MANIFOLD_DIM[MANIS[name]] < 2 or geom == "t2_noxs"):
                    continue  # (partial densities need dimension >= 2; partial batches run the generic kernels with or without _xs)
                for F in (2, 3, 4):
                    for niter in (1, 3):
                        out.append((geom, name, "partial" if partial else "full", F, niter))
    return out


@pytest.mark.parametrize("geom,name,inputs,F,niter", _cases(), ids=lambda v: str(v))
def test_points_and_labels_equal_the_oracle(geom, name, inputs, F, niter, oracle_backend, monkeypatch):
    N, n, env = GEOMS[geom]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read when the context is created)
    specs = _specs(name, F, n, inputs == "partial")
    keep = sorted({0, 1, 2, n // 2, n - 1} & set(range(n)))  # every mask pattern, the middle and the end of the batch
    ran = {}
    pts, labs = run(lambda *a: _WithNiter(hip(*a), niter), N, specs, plans=ran)
    _assert_geometry(geom, name, inputs == "partial", F, ran["product"])
    opts, olabs = run(lambda *a: _WithNiter(oracle_backend(*a), niter), N, specs, keep=keep)
    for i in range(n):
        assert np.isfinite(pts[i]).all(), f"product {i}"
        assert labs[i].min() >= 0 and labs[i].max() < N, f"product {i}: label out of range"
    for i in keep:
        assert np.array_equal(labs[i], olabs[i]), f"product {i}: labels differ from the oracle's"
        assert np.array_equal(pts[i], opts[i]), f"product {i}: points differ from the oracle's"


@pytest.mark.parametrize("form", ["p2", "p1"])
@pytest.mark.parametrize("niter", [1, 3])
@pytest.mark.parametrize("F", [2, 3, 4])
def test_fused_update_equals_the_oracle(F, niter, form, oracle_backend, hip_backend, monkeypatch):
    monkeypatch.setenv("NBP_FUSED_MIN", "16")
    if form == "p1":
        monkeypatch.setenv("NBP_FUSED_P1_MIN", "1")  # one lane per particle, the form of rounds that fill the chip
    nops = 24
    rng = np.random.default_rng(9)
    src = [rand_points(rng, FUSED_MAN, FUSED_N, c, 0.4) for c in (0.0, 2.0, 1.0)]
    props, prods, stride = _round(nops, F)
    for d in prods:
        d.niter = niter
    res = []
    for make in (oracle_backend, hip_backend):
        be = make(FUSED_N, 4 + stride * nops, 0)
        for s, p in enumerate(src):
            be.slot_write(s, FUSED_MAN, p)
        prog = be.program([(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)])
        if make is hip_backend:
            assert prog.num_fused() == 1
        prog.run()
        be.synchronize()
        res.append([be.slot_read(4 + stride * i + F, FUSED_MAN) for i in range(nops)])
        prog.close()
        be.close()
    for i, ((p, bw), (q, bw2)) in enumerate(zip(*res)):
        assert np.array_equal(q, p), f"update {i}: points differ from the oracle's"
        assert np.array_equal(bw2, bw), f"update {i}: bandwidth differs from the oracle's"
