"""-m gpu: a product LAUNCH that mixes density counts, where the node statistics do not fit the LDS and live in the launch's
global scratch ("big": 3-D manifolds from ~260 particles on with four densities, or many densities at fewer particles).
The scratch of a workgroup is addressed by the LAUNCH's largest density count -- addressed by the product's own, as it was
through round 5, the workgroups wrote over each other's statistics and products came out wrong or non-finite (found by the
whole-solve differential check of round 5 on an SE(2) lattice at N = 300: tools/exp/whole_solve_sha_se2.sh).  Every product of
the launch that is compared must be the oracle's.

Whether a launch is big is read from the plan it recorded (HipBackend.last_plans) and asserted.  Two of the shapes (N = 320 with up
to four densities in the latency geometry) turned out to keep their statistics in LDS -- they stay, as launches that mix density
counts on the single-manifold kernels, and the same launches with five densities, which are big, stand beside them."""
import numpy as np
import pytest

from parity_utils import abi, iif, product_desc, rand_points

pytestmark = pytest.mark.gpu


def run(make, N, man, Fs, keep=None, nsrc=16, plans=None):
    nprod = len(Fs)
    be = make(N, nsrc + nprod)
    try:
        rng = np.random.default_rng(1)
        for j in range(nsrc):
            be.slot_write(j, man, rand_points(rng, man, N, 0.2 * j, 0.3))
        be.run_bandwidth(list(range(nsrc)), [man] * nsrc)
        descs = [product_desc(man, [(3 * i + j) % nsrc for j in range(Fs[i])], nsrc + i, 5 + i) for i in range(nprod)]
        if keep is not None:  # the oracle: only the products that are compared (each is independent of the others)
            descs = [descs[i] for i in keep]
        be.run_products(descs)
        if plans is not None:
            plans.update(be.last_plans())
        return {i: be.slot_read(nsrc + i, man)[0] for i in (keep if keep is not None else range(nprod))}
    finally:
        be.close()


# the launches whose node statistics stay in LDS (8 helper lanes, no chunk sums: four densities at N = 320 fit -- the
# single-manifold kernels nbp_product_kernel_l8_se / _l8_e3); every other launch here is big
IN_LDS = {(abi.SE2, 320, 120, (2, 3, 4)), (abi.EUCLID3, 320, 40, (2, 3, 4))}


@pytest.mark.parametrize("man,N,nprod,counts", [
    (abi.SE2, 300, 332, (2, 3, 4)),      # the launch that failed: a tree level of an SE(2) lattice, throughput geometry asked for
    (abi.SE2, 320, 120, (2, 3, 4)),
    (abi.EUCLID3, 300, 332, (2, 3, 4)),
    (abi.EUCLID3, 320, 40, (2, 3, 4)),
    (abi.SE2, 200, 60, (2, 5, 9)),       # many densities at BASELINE's particle count
    (abi.EUCLID2, 300, 250, (2, 4, 12)),
    (abi.CIRCULAR, 200, 30, (2, 7, 20)),
    (abi.SE2, 320, 120, (2, 3, 5)),      # the two launches of IN_LDS with a fifth density: big
    (abi.EUCLID3, 320, 40, (2, 3, 5)),
])
def test_products_of_a_launch_that_mixes_density_counts_are_the_oracles(oracle_backend, hip_backend, man, N, nprod, counts):
    big = (man, N, nprod, counts) not in IN_LDS
    Fs = [counts[2] if i % 9 == 8 else (counts[1] if i % 17 == 3 else counts[0]) for i in range(nprod)]
    keep = [i for i in range(nprod) if Fs[i] != counts[0]][:6] + list(range(4))
    ran = {}
    d = run(hip_backend, N, man, Fs, plans=ran)
    plan = ran["product"]
    assert (plan["status"], plan["N"], plan["n"], plan["F"], plan["big"]) == (0, N, nprod, counts[2], int(big)), plan
    if big:  # the scratch path: eight helper lanes, a generic kernel, the launch's own stride (nbp_product_gstats_doubles(F, 3, N))
        assert plan["HL"] == 8 and plan["row_mani"] == 0 and plan["gstats"] == nprod * plan["G"] * 12 * counts[2] * N, plan
    o = run(oracle_backend, N, man, Fs, keep=keep)
    assert all(np.isfinite(v).all() for v in d.values())
    for i in keep:
        np.testing.assert_allclose(d[i], o[i], rtol=0, atol=0, err_msg=f"product {i} ({Fs[i]} densities)")
