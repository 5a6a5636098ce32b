"""-m gpu: a product launch in a latency geometry (fewer than NBP_PRODUCT_HL2_MIN products: 32 or 8 helper lanes per sample)
whose multi-density products share one manifold, have only full inputs and keep their node statistics in LDS runs a
single-manifold instance (nbp_product_kernel_{y32,l8}_{e1,e2,e3,ci,se}); partial, mixed and big launches run the generic
kernels.  Both run the same product_body, so the points and the labels must be the oracle's and the generic kernel's, bit for
bit.  The generic leg runs in a child process with NBP_NO_UNIFORM_LATENCY_PRODUCTS set (the library reads it once).

Which kernel a launch ran is read from the plan it recorded (HipBackend.last_plans) and asserted for both legs: a case that a
moved threshold sends to another kernel fails instead of passing on it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity_utils import ROOT, abi, iif, rand_points

pytestmark = pytest.mark.gpu

MANIS = {"e1": abi.EUCLID1, "e2": abi.EUCLID2, "e3": abi.EUCLID3, "ci": abi.CIRCULAR, "se": abi.SE2}
# (N, products, densities): y32 with one and with fifteen products; l8 with at most 256 workgroups (N = 200: seven per
# product, where the generic kernels take their `_w1` form) and with more (N = 300: ten per product)
SHAPES = [(64, 1, 8), (300, 1, 2), (200, 15, 3), (200, 36, 2), (300, 60, 3), (64, 40, 8)]
NSRC = 12


def cases():
    out = {}
    for name, man in MANIS.items():
        for N, n, F in SHAPES:
            out[f"{name}_N{N}_n{n}_F{F}"] = (N, [(man, F, None)] * n)
    # a partial input in every third product: the generic kernel (the partial bodies)
    for name in ("e2", "e3", "se"):
        man, D = MANIS[name], abi.MANIFOLD_DIM[MANIS[name]]
        out[f"partial_{name}"] = (200, [(man, 3, [1, 0, (1 << D) - 2] if i % 3 == 1 else None) for i in range(12)])
    # two manifolds in one launch: the generic kernel
    out["mixed_e2_se"] = (200, [(abi.EUCLID2 if i % 2 else abi.SE2, 2 + i % 3, None) for i in range(20)])
    out["mixed_e1_ci"] = (64, [(abi.EUCLID1 if i % 3 else abi.CIRCULAR, 3, None) for i in range(5)])
    return out


def run(make, N, specs, keep=None, plans=None):
    """-> ({product: points}, {product: labels}) of the products in `keep` (all by default); `plans` (a dict) receives what the
    launches of the batch recorded (HipBackend.last_plans)"""
    manis = sorted({m for m, _, _ in specs})
    base = {m: k * (NSRC + 1) for k, m in enumerate(manis)}  # NSRC sources of each manifold + one slot of old points
    out0 = len(manis) * (NSRC + 1)
    Fmax = max(F for _, F, _ in specs)
    be = make(N, out0 + len(specs), len(specs) * N * Fmax + 16)
    try:
        rng = np.random.default_rng(7)
        for m in manis:
            for j in range(NSRC + 1):
                be.slot_write(base[m] + j, m, rand_points(rng, m, N, 0.2 * j, 0.3))
            be.run_bandwidth(list(range(base[m], base[m] + NSRC + 1)), [m] * (NSRC + 1))
        descs = [iif.solver.product_desc(m, [base[m] + (3 * i + j) % NSRC for j in range(F)], out0 + i, 11 + i, 1, i * N * Fmax,
                                         partials=parts, old_slot=base[m] + NSRC)
                 for i, (m, F, parts) in enumerate(specs)]
        idx = list(range(len(specs))) if keep is None else keep
        be.run_products([descs[i] for i in idx])  # each product depends on its own descriptor only
        if plans is not None:
            plans.update(be.last_plans())
        pts = {i: be.slot_read(out0 + i, specs[i][0])[0] for i in idx}
        labs = {i: np.array(be.side_read(i * N * Fmax, N * specs[i][1])) for i in idx}
        return pts, labs
    finally:
        be.close()


GENERIC_PLAN = ("HL", "row_mani", "w1", "big", "n", "G")  # what the generic leg hands back of its recorded plans


def expected_plan(key, N, specs):
    """what the docstring says the launch of a case runs: (helper lanes, kernel of the single-manifold leg, `_w1` of the generic leg)"""
    n = len(specs)
    HL = 32 if n < 16 else 8
    geom = "y32" if HL == 32 else "l8"
    uniform = key.split("_")[0] in MANIS
    G = -(-(-(-N // (64 // HL))) // 4)  # workgroups of four waves per product
    w1 = n * G <= 256  # at most one workgroup per CU: the generic kernels take their `_w1` form
    return HL, f"nbp_product_kernel_{geom}_{key.split('_')[0]}" if uniform else f"nbp_product_kernel_{geom}" + ("_w1" if w1 else ""), w1


def hip(N, n_slots, side_ints):
    return iif.HipBackend(N, n_slots, side_ints=side_ints)


def _generic_leg(path):
    """(child process, NBP_NO_UNIFORM_LATENCY_PRODUCTS set) every case on the generic kernels -> one .npz"""
    arrs = {}
    for key, (N, specs) in cases().items():
        ran = {}
        pts, labs = run(hip, N, specs, plans=ran)
        arrs[f"{key}/plan"] = np.array([ran["product"][k] for k in GENERIC_PLAN])
        for i in pts:
            arrs[f"{key}/p{i}"] = pts[i]
            arrs[f"{key}/l{i}"] = labs[i]
    np.savez(path, **arrs)


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("generic") / "generic.npz")
    code = (f"import sys; sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {ROOT!r}]; "
            f"import test_gpu_latency_product_instances as t; t._generic_leg({path!r})")
    env = dict(os.environ, NBP_NO_UNIFORM_LATENCY_PRODUCTS="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(path))


@pytest.mark.parametrize("key", list(cases()))
def test_latency_products_equal_oracle_and_generic_kernel(key, generic, oracle_backend):
    N, specs = cases()[key]
    ran = {}
    pts, labs = run(hip, N, specs, plans=ran)
    HL, kernel, w1 = expected_plan(key, N, specs)
    plan, gplan = ran["product"], dict(zip(GENERIC_PLAN, generic[f"{key}/plan"]))
    assert (plan["status"], plan["HL"], plan["kernel"], plan["big"], plan["n"]) == (0, HL, kernel, 0, len(specs)), plan
    assert (gplan["HL"], gplan["row_mani"], gplan["w1"], gplan["big"], gplan["n"]) == (HL, 0, int(w1), 0, len(specs)), gplan
    if key.endswith("_N200_n36_F2"):   # (SHAPES: at most 256 workgroups, the generic kernels in their `_w1` form ...
        assert gplan["w1"] == 1 and gplan["n"] * gplan["G"] == 252
    if key.endswith("_N300_n60_F3"):   #  ... and more)
        assert gplan["w1"] == 0 and gplan["n"] * gplan["G"] == 600
    keep = sorted({0, len(specs) // 2, len(specs) - 1} | {i for i in range(len(specs)) if specs[i][2] is not None or specs[i][0] != specs[0][0]})[:6]
    opts, olabs = run(lambda n, s, si: oracle_backend(n, s, si), N, specs, keep=keep)
    for i in range(len(specs)):
        assert np.isfinite(pts[i]).all(), f"product {i}"
        assert np.array_equal(pts[i], generic[f"{key}/p{i}"]), f"product {i}: points differ from the generic kernel's"
        assert np.array_equal(labs[i], generic[f"{key}/l{i}"]), f"product {i}: labels differ from the generic kernel's"
    for i in keep:
        assert np.array_equal(pts[i], opts[i]), f"product {i}: points differ from the oracle's"
        assert np.array_equal(labs[i], olabs[i]), f"product {i}: labels differ from the oracle's"
