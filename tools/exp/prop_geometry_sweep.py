"""launch times of the three Euclid(2) proposal geometries (workgroup, one wave, two waves per proposal) at B proposals of N = 200 -- the batch
of prop_batch.py lin2, 7 single launches per geometry, one process: prop_geometry_sweep.py [B ...]"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
from parity_utils import abi, iif, rand_points, relative_factor_desc
N, REPS = 200, 7
MODES = {"workgroup": {"NBP_PROPOSAL_WAVE_MIN": "100000000", "NBP_PROPOSAL_SPLIT_MIN": "100000000"}, "wave": {"NBP_PROPOSAL_WAVE_MIN": "1"},
         "split2": {"NBP_PROPOSAL_WAVE_MIN": "100000000", "NBP_PROPOSAL_SPLIT_MIN": "1"}}
KEYS = ("NBP_PROPOSAL_WAVE_MIN", "NBP_PROPOSAL_SPLIT_MIN")
Bs = [int(a) for a in sys.argv[1:]] or [128, 245, 350, 488, 700, 975, 1463, 2000, 4000]
print(f"{'B':>5s} {'mode':10s} {'min':>7s} {'median':>7s} {'max':>7s}  us per launch, {REPS} single launches; launches by geometry (wg, wave, split); residual evals")
for B in Bs:
    rng = np.random.default_rng(0)
    pts = [rand_points(rng, abi.EUCLID2, N, 3.0 + j, 0.3) for j in range(B + 1)]
    ref = None
    for mode, env in MODES.items():
        for k in KEYS: os.environ.pop(k, None)
        os.environ.update(env)
        be = iif.HipBackend(N, 2 * B + 2, 0)
        for k in KEYS: os.environ.pop(k, None)
        for j in range(B + 1): be.slot_write(j, abi.EUCLID2, pts[j])
        descs = []
        for j in range(B):
            d = relative_factor_desc(abi.F_LINREL, abi.EUCLID2, 2, 1, [j, j + 1], B + 1 + j, 5 + j, [1.0, 0.0], [0.1, 0.1]); d.skip_bandwidth = 1
            descs.append(d)
        be.run_proposals(descs); be.timing_enable(True); be.timing_read(); be.diag(reset=True)
        ts = []
        for _ in range(REPS):
            be.run_proposals(descs)
            ts.append(be.timing_read()["nbp_proposal_kernel"][0] * 1e3)
        dg = be.diag()
        out = be.slot_read(B + 1 + B // 2, abi.EUCLID2)[0]
        if ref is None: ref = out
        same = np.array_equal(ref, out)
        ts.sort()
        print(f"{B:5d} {mode:10s} {ts[0]:7.1f} {ts[len(ts) // 2]:7.1f} {ts[-1]:7.1f}  ({dg['proposal_launches_workgroup']}, {dg['proposal_launches_wave']}, {dg['proposal_launches_split']}) {dg['residual_evals'] // REPS} same_as_workgroup={same}", flush=True)
        be.close()
