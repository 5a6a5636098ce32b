"""latency product launches of one manifold, time per launch by the library's timing events (A/B of the single-manifold latency instances: NBP_LIB_OVERRIDE / NBP_NO_UNIFORM_LATENCY_PRODUCTS).  Usage: latency_products.py TAG"""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
from parity_utils import abi, iif, product_desc, rand_points
tag = sys.argv[1]
cases = [(abi.EUCLID2, 200, 1, 2), (abi.EUCLID2, 200, 11, 2), (abi.EUCLID2, 200, 11, 3), (abi.EUCLID2, 200, 36, 2), (abi.EUCLID2, 200, 47, 2),
         (abi.EUCLID2, 200, 69, 2), (abi.EUCLID3, 200, 47, 2), (abi.SE2, 200, 11, 3), (abi.SE2, 200, 47, 2), (abi.CIRCULAR, 200, 47, 2)]
for man, N, nprod, F in cases:
    be = iif.HipBackend(N, 64 + nprod, 0)
    rng = np.random.default_rng(0)
    for j in range(64):
        be.slot_write(j, man, rand_points(rng, man, N, 1.0 + 0.1 * j, 0.3))
    be.run_bandwidth(list(range(64)), [man] * 64)
    descs = [product_desc(man, [(3 * i + j) % 64 for j in range(F)], 64 + i, 5 + i) for i in range(nprod)]
    be.run_products(descs)
    be.timing_enable(True); be.timing_read()
    reps = 30
    for _ in range(reps): be.run_products(descs)
    t = be.timing_read()
    us = {k: round(v[0] / reps * 1e3, 1) for k, v in t.items() if v[0] > 0}
    print(json.dumps({"lib": tag, "mani": man, "N": N, "nprod": nprod, "F": F, "us": us}), flush=True)
    be.close()
