"""-m "not gpu": what the fused update kernel's cases (tests/fused_cases.py) establish without a device.  Every case runs on
the oracle alone and leaves what a variable update must leave -- N finite points, positive bandwidths, infoPerCoord = F on
both coordinates (ones for a single density) -- and the host-side restatement of the kernel's LDS need, by which the
device leg decides whether a round must fuse, is held to nbp_update_lds_bytes as the compiler sees it."""
import os
import subprocess

import numpy as np
import pytest

import fused_cases as fc
from parity_utils import ROOT

CASES = fc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_on_the_oracle(case, oracle_backend):
    r = case.run(oracle_backend)
    assert r["nf"] is None
    for pts, bw, ipc in r["out"][:case.nops]:
        assert pts.shape == (case.out_count, 2)  # the count field reads "N points" (a lone kept pass-through: the density's)
        assert np.isfinite(pts).all()
        assert np.isfinite(bw).all() and (bw > 0).all()
        assert np.array_equal(ipc, np.full(2, float(case.F) if case.F > 1 else 1.0))
    for pts, bw, ipc in r["prop"]:
        assert pts.shape[1] == 2 and np.isfinite(pts).all()
    for pts, bw, ipc in r["out"][case.nops:]:  # (copies of proposals)
        assert pts.shape == (case.N, 2) and np.isfinite(pts).all() and (bw > 0).all()


def test_every_recipe_is_used():
    used = {name for c in CASES for name in c.recipes}
    assert used == set(fc.RECIPES)


def test_the_legacy_round_is_unchanged():
    """`_round` of the earlier tests (imported by test_gpu_product_first_label.py): same slots, kinds and seeds"""
    props, prods, stride = fc.legacy_round(3, 3)
    assert stride == 4 and [d.out_slot for d in prods] == [7, 11, 15] and [d.seed for d in prods] == [5000, 5001, 5002]
    assert [d.out_slot for d in props] == [4, 5, 6, 8, 9, 10, 12, 13, 14]
    assert [d.factor_kind for d in props[:3]] == [fc.abi.F_LINREL, fc.abi.F_LINREL, fc.abi.F_PRIOR]
    assert [list(d.var_slot)[:2] for d in props[:3]] == [[0, 2], [1, 2], [2, 0]]
    assert [d.seed for d in props[3:6]] == [907, 908, 909]
    assert fc.legacy_round(2, 1)[0][0].factor_kind == fc.abi.F_LINREL


def test_lds_formula_equals_the_header(tmp_path):
    """fc.lds_bytes against nbp_update_lds_bytes of csrc/nbp_fused.h, evaluated by a host program that includes the header"""
    csrc = os.path.join(ROOT, "incrementalinference.jl_amd", "csrc")
    src = tmp_path / "lds.hip"
    src.write_text('#include <cstdio>\n#include "nbp_fused.h"\n'
                   'int main() { int F, N, P, c; while (scanf("%d %d %d %d", &F, &N, &P, &c) == 4) '
                   'printf("%zu\\n", nbp_update_lds_bytes(F, c ? 1 : 2, N, (N + 63) / 64 * 64, P, c != 0)); return 0; }\n')
    exe = tmp_path / "lds"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O0", "-std=c++17", "-DNBP_TU=0",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, str(src), "-o", str(exe)])
    q = [(F, N, P, c) for F in (2, 3, 4) for N in (8, 37, 64, 65, 128, 129, 200, 256) for P in (1, 2) for c in (0, 1)]
    got = subprocess.check_output([str(exe)], input="".join("%d %d %d %d\n" % t for t in q).encode()).split()
    assert len(got) == len(q)
    for (F, N, P, c), g in zip(q, got):
        assert fc.lds_bytes(F, 1 if c else 2, N, fc.npad(N), P, bool(c)) == int(g), (F, N, P, c)
    # every size the device leg runs is under the ceiling, the library's largest fusable shape included: no (N, F) falls back
    assert all(fc.admits(N, F) for N in fc.SIZES for F in fc.SIZE_F)
    assert not any(fc.admits(N, F) for N in fc.SIZES_REFUSED for F in fc.SIZE_F)
