"""CPU: the launch plans of the library over their whole argument space.

What a product launch runs -- helper lanes, workgroup, workgroups per product, LDS or global node statistics, `_xs`, chunks per
helper range, resident levels, `_w1`, the wide workgroups, the row of the kernel table, the dynamic LDS size -- is decided on the host
by product_plan (csrc/nbp_api.hip); the kernel then lays out that LDS on its own (product_lds_layout, nbp_kernels.h).  fit_plan
does the same for the bandwidth fits, proposal_plan for the proposals.  A plan and its kernel that disagree do not fault: an LDS
overrun gives wrong or non-finite posteriors, found late, by whole solves.

The plans are read through the plan queries of the C ABI (nbp_plan_products / nbp_plan_fits / nbp_plan_proposals: the planners
themselves on a context that holds only what they read -- no GPU).  launch_plan_check.cpp, compiled here against the kernels' own
header, sweeps the whole space (217 million product plans: every N in 8..512 and F in 1..128 under eight option sets) and holds every
plan to its invariants; its counts are printed.  The other tests check the query itself and the case list of
test_gpu_launch_plan_coverage.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import launch_plan_cases as lpc
from parity_utils import ROOT, abi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "incrementalinference.jl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return abi.load_library()


def kernel_table_rows():
    src = open(os.path.join(CSRC, "nbp_api.hip")).read()
    table = src[src.index("NBP_PRODUCT_KERNELS[] = {"):]
    return re.findall(r"NBP_ROW\((nbp_product_kernel_\w+),", table[:table.index("};")])


@pytest.fixture(scope="module")
def sweep(lib, tmp_path_factory):
    """the stand-alone checker, compiled from the project's own headers and run once over the whole space -> its output"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("plans") / "launch_plan_check")
    # (a HIP program for the host alone: nbp_kernels.h declares the kernels, NBP_TU = 0 compiles none of them)
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wno-unused-value", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(HERE, "launch_plan_check.cpp"), "-o", exe, "-ldl"], check=True)
    with lpc.options({}):
        out = subprocess.run([exe, os.environ.get("NBP_LIB_OVERRIDE") or abi.LIB_PATH, str(len(kernel_table_rows()))], capture_output=True, text=True)
    print(out.stdout)
    return out


def test_every_plan_of_the_whole_space_holds_its_invariants(sweep):
    """Every product plan: NBP_OK with a kernel or a defined refusal, never "no kernel" where the LDS fits; every row of the table
    chosen; lds <= 160 KB and at least what the chosen kernel addresses for every product of 2 .. F densities; the workgroup within
    the kernel's launch bound, a multiple of four waves in the throughput geometry; G * SPB >= N > (G - 1) * SPB; big only with eight
    helper lanes on a generic row, its scratch n * G * nbp_product_gstats_doubles(F, 3, N), refused inside a round; _w1 only up
    to 256 workgroups of four waves outside a round; a half of a round under the geometry of its whole batch.  Every fit plan:
    threads, w5, depth, LDS.  Every proposal plan: wave and split for simple Euclid(2) / Euclid(3) batches within their N, LDS
    under the cap.  (launch_plan_check.cpp says how each is checked, and which invariants had to be corrected: DESIGN.md 8.)"""
    assert sweep.returncode == 0, sweep.stdout[-6000:] + sweep.stderr[-2000:]
    m = re.search(r"products total: (\d+) plans checked, (\d+) launched, (\d+) distinct signatures, (\d+) refusals", sweep.stdout)
    # the full sweep, not a sample: 505 N x 10 n x 128 F x 3 D x 7 mani x 2 geom_n x 8 option sets
    assert m and int(m.group(1)) == 505 * 10 * 128 * 3 * 7 * 2 * 8, sweep.stdout[-2000:]
    assert int(m.group(2)) > 0 and int(m.group(3)) > 0
    assert re.search(r"fits total: (\d+) plans checked", sweep.stdout) and re.search(r"proposals total: (\d+) plans checked", sweep.stdout)
    assert "ok: 0 failures" in sweep.stdout


def test_no_plan_allocates_more_lds_than_its_kernel_addresses(sweep):
    """equality, apart from the lower bound: `lds` is exactly the need of the largest product of the launch (an oversize plan
    quietly costs residency)"""
    m = re.search(r"(\d+) oversize plans", sweep.stdout)
    assert m and int(m.group(1)) == 0, sweep.stdout[-3000:]


def test_plan_structs_match_the_header(tmp_path):
    names = ["nbp_product_plan_req", "nbp_product_plan_rec", "nbp_fit_plan_req", "nbp_fit_plan_rec", "nbp_proposal_plan_req", "nbp_proposal_plan_rec"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbp.h"\nint main(){printf("' + "%zu " * (len(names) + 4) + '\\n",' +
                   ",".join(f"sizeof({n})" for n in names) +
                   ",offsetof(nbp_product_plan_rec,lds),offsetof(nbp_product_plan_rec,kernel),offsetof(nbp_fit_plan_rec,lds),offsetof(nbp_proposal_plan_rec,lds));return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(t) for t in (abi.ProductPlanReq, abi.ProductPlanRec, abi.FitPlanReq, abi.FitPlanRec, abi.ProposalPlanReq, abi.ProposalPlanRec)] + \
           [abi.ProductPlanRec.lds.offset, abi.ProductPlanRec.kernel.offset, abi.FitPlanRec.lds.offset, abi.ProposalPlanRec.lds.offset]
    assert got == want


def test_the_query_reads_the_environment_as_a_context_does(lib):
    q = (200, 500, 3, 2, abi.EUCLID2, 0)
    with lpc.options({}):
        d = abi.plan_products([q])[0].as_dict()
    assert (d["status"], d["HL"], d["xs"], d["kernel"]) == (0, 2, 1, "nbp_product_kernel_t2_e2_xs")
    with lpc.options({"NBP_NO_XS_PRODUCTS": "1"}):
        assert abi.plan_products([q])[0].kernel == b"nbp_product_kernel_t2_e2"
    with lpc.options({"NBP_PRODUCT_NCH": "1"}):
        assert abi.plan_products([q])[0].nch == 1
    with lpc.options({"NBP_PRODUCT_HL2_MIN": "1000"}):
        assert abi.plan_products([q])[0].HL == 8
    with lpc.options({}):
        assert abi.plan_products([q])[0].as_dict() == d  # and nothing of it stays behind
        assert abi.plan_fits([(200, 1, 2, 0, 0, 0)])[0].depth == 3
    with lpc.options({"NBP_NO_SPECULATIVE_FITS": "1"}):
        assert abi.plan_fits([(200, 1, 2, 0, 0, 0)])[0].depth == 0
    # arguments no launch has are refused, not planned
    with pytest.raises(ValueError):
        abi.plan_products([(7, 1, 2, 2, abi.EUCLID2, 0)])
    with pytest.raises(ValueError):
        abi.plan_products([(200, 1, 129, 2, abi.EUCLID2, 0)])
    assert abi.plan_products([(200, 1, 2, 3, abi.EUCLID2, 0)])[0].status == -1  # NBP_ERR_ARG: D is not Euclid(2)'s


def test_plans_the_other_product_tests_rely_on(lib):
    """the shapes by which test_gpu_product_first_label.py, test_gpu_latency_product_instances.py and
    test_gpu_mixed_product_launches.py mean to reach a geometry (they assert the recorded plan on the GPU; here the same plans fail
    without one when a threshold moves)"""
    with lpc.options({}):
        def plan(N, n, F, D, mani):
            return abi.plan_products([(N, n, F, D, mani, 0)])[0]
        assert plan(200, 1, 2, 2, abi.EUCLID2).kernel == b"nbp_product_kernel_y32_e2"
        assert plan(200, 40, 3, 3, abi.SE2).kernel == b"nbp_product_kernel_l8_se"
        assert plan(200, 500, 4, 1, abi.CIRCULAR).kernel == b"nbp_product_kernel_t2_ci_xs"
        assert plan(200, 500, 3, 3, 0).kernel == b"nbp_product_kernel_t2"               # partial inputs: the generic kernel
        r = plan(512, 200, 4, 3, abi.SE2)                                              # big: eight helper lanes, generic, scratch
        assert (r.big, r.HL, r.kernel, r.gstats > 0) == (1, 8, b"nbp_product_kernel_l8", True)
        r = plan(512, 200, 2, 2, abi.EUCLID2)                                          # two densities fit: one wide workgroup
        assert (r.big, r.wpb, r.G, r.kernel) == (0, 16, 1, b"nbp_product_kernel_t2_e2_xs")
        # one workgroup per CU at most: the generic latency kernels take their `_w1` form (N = 200: seven workgroups per product)
        assert plan(200, 36, 2, 3, 0).kernel == b"nbp_product_kernel_l8_w1" and plan(200, 37, 2, 3, 0).kernel == b"nbp_product_kernel_l8"
        assert plan(200, 20, 4, 3, 0).w1 == 1 and plan(64, 5, 3, 1, 0).kernel == b"nbp_product_kernel_y32_w1"
        assert plan(200, 12, 3, 3, 0).kernel == b"nbp_product_kernel_y32"  # (twelve products of 25 workgroups: 300)


def test_the_gpu_case_list_covers_every_signature_and_every_row(lib):
    cases = lpc.product_cases()
    covered = {c["sig"] for c in cases}
    default_sigs = {sig for oname, _, sig in lpc.product_candidates() if oname == "defaults"}
    assert default_sigs and default_sigs <= covered, default_sigs - covered
    assert {sig for _, _, sig in lpc.product_candidates()} == covered
    assert {c["plan"]["kernel"] for c in cases} == set(kernel_table_rows())
    assert len({c["id"] for c in cases}) == len(cases)
    for kind, N, n, F, oname in lpc.BIG_UNDER_HL2_MIN:  # the launches of the bug the sweep found: big, and on the scratch path now
        plan = next(c["plan"] for c in cases if c["id"] == f"{kind}_N{N}_n{n}_F{F}_{oname}")
        assert (plan["big"], plan["HL"], plan["row_mani"]) == (1, 8, 0) and plan["kernel"].startswith("nbp_product_kernel_l8"), plan
    fits = lpc.fit_cases()
    kernels = {c["plan"]["kernel"] for c in fits}
    assert {"nbp_bandwidth_kernel", "nbp_bandwidth_kernel_w5", "nbp_bandwidth_kernel_spec<2>", "nbp_bandwidth_kernel_spec<3>", "nbp_prep_kernel",
            "nbp_prep_kernel_w5", "nbp_prep_kernel_spec<2>", "nbp_prep_kernel_spec<3>"} == kernels
    for P in (2, 4):  # each with the depths 0, 2 and 3
        assert {c["plan"]["depth"] for c in fits if c["plan"]["P"] == P and not c["plan"]["prep"]} == {0, 2, 3}
    # a condition, not a measurement: beyond it the candidate shapes are coarsened, never the signature
    assert len(cases) + len(fits) <= lpc.MAX_CASES, (len(cases), len(fits))
    print(f"{len(cases)} product cases, {len(fits)} fit cases")
