"""The GPU cases of tests/test_gpu_launch_plan_coverage.py, computed with the plan queries of the library (abi.plan_products /
abi.plan_fits: no context, no GPU): for every plan SIGNATURE the candidate shapes reach, the smallest candidate that reaches it.
tests/test_launch_plans.py checks the list on the CPU (every signature of the default options, every row of the kernel table,
at most MAX_CASES cases).

A product plan's signature is (row of the kernel table, big, nch, all_levels, wpb, G > 1, circ); a fit plan's is (kernel, P, depth,
w5) -- the kernel's name says prep or plain launch."""
import contextlib
import functools
import os

from parity_utils import abi

MAX_CASES = 200

# every switch the planners read: a context (or a query) under an option set has exactly that set
PLAN_VARS = ("NBP_PRODUCT_HL2_MIN", "NBP_PRODUCT_NCH", "NBP_PRODUCT_ALL_LEVELS_HL", "NBP_NO_XS_PRODUCTS", "NBP_NO_UNIFORM_LATENCY_PRODUCTS",
             "NBP_NO_SPECULATIVE_FITS", "NBP_SPEC_DEPTH3", "NBP_LCV_P2_MIN", "NBP_LCV_P1_MIN", "NBP_NO_W5_FITS",
             "NBP_PROPOSAL_WAVE_MIN", "NBP_PROPOSAL_SPLIT_MIN")
OPTION_SETS = {
    "defaults": {},
    "hl2min1": {"NBP_PRODUCT_HL2_MIN": "1"},
    "nch1": {"NBP_PRODUCT_NCH": "1"},
    "nch8": {"NBP_PRODUCT_NCH": "8"},
    "nch15": {"NBP_PRODUCT_NCH": "15"},
    "alllevels2": {"NBP_PRODUCT_ALL_LEVELS_HL": "2"},
    "noxs": {"NBP_NO_XS_PRODUCTS": "1"},
    "nolatuni": {"NBP_NO_UNIFORM_LATENCY_PRODUCTS": "1"},
}
FIT_OPTION_SETS = {"defaults": {}}

PARTICLES = (64, 65, 130, 200, 257, 300, 320, 512)
DENSITIES = (2, 3, 4, 8, 40)
MANIS = {"e1": abi.EUCLID1, "e2": abi.EUCLID2, "e3": abi.EUCLID3, "ci": abi.CIRCULAR, "se": abi.SE2}
KINDS = tuple(MANIS) + ("mixed", "partial")
# products per launch: one or two and 15 (the latency geometry of 32 helper lanes, with at most and -- from N = 137 on -- with more
# than 256 workgroups: the `_w1` kernels and the plain ones), 16 / 17 / 37 / 129 (8 helper lanes on either side of 256 workgroups
# at 16, 7 and 2 workgroups per product), 192 (NBP_PRODUCT_HL2_MIN: the throughput geometry)
PRODUCTS = (15, 16, 17, 37, 129, 192)
# fits per launch: the depths of the speculation (1: three iterations per rendezvous, 20 on Euclid(2): two, 41: none), more than
# NBP_LCV_P2_MIN / NBP_LCV_P1_MIN workgroups (129, 513)
FITS = (1, 20, 41, 129, 513)
FIT_MANIFOLD = abi.EUCLID2
# updates of a program's round (two proposals and a product of two densities each): the prep launch runs the 2 x ROUNDS fits of
# the proposals beside the KD builds -- speculation of depth three, of depth two, none
ROUNDS = (1, 8, 21)


@contextlib.contextmanager
def options(env):
    """the environment with exactly the planner switches of `env` (put back afterwards): what a context created or a plan queried
    inside reads"""
    saved = {k: os.environ.pop(k, None) for k in PLAN_VARS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in PLAN_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def product_specs(kind, n, F):
    """the batch of a case as the harness of test_gpu_latency_product_instances.py takes it: (manifold, densities, partial masks)
    per product.  A batch whose largest count is three or more holds a product of TWO densities at index 1 (a launch that mixes
    density counts: the scratch stride of the big kernels is the launch's, not the product's)."""
    out = []
    for i in range(n):
        man = MANIS[kind] if kind in MANIS else (abi.SE2 if kind == "partial" or i % 2 == 0 else abi.EUCLID2)
        Fi = 2 if (F >= 3 and i == 1) else F
        parts = ([1, 0, 6] + [0] * F)[:Fi] if (kind == "partial" and i % 3 == 0) else None  # x only + full + (y, theta): SE(2)
        out.append((man, Fi, parts))
    return out


def product_query(kind, N, n, F):
    """(N, n, F, D, mani, geom_n) of the launch of product_specs(kind, n, F): what products_maxfd / products_uniform_manifold
    make of it"""
    if kind in MANIS:
        return (N, n, F, abi.MANIFOLD_DIM[MANIS[kind]], MANIS[kind], 0)
    return (N, n, F, 3, 0, 0)  # two manifolds, or partial inputs: the generic kernels, sized by SE(2)


def product_keep(n, F):
    """the products compared with the oracle: the first, the middle, the last, and the two-density one"""
    return sorted({0, n // 2, n - 1} | ({1} if F >= 3 else set()))


def product_signature(r):
    return (r.row, r.big, r.nch, r.all_levels, r.wpb, int(r.G > 1), r.circ)


def fit_signature(r):
    return (r.kernel.decode(), r.P, r.depth, r.w5)


def _smallest(cands):
    """{signature: (size, case)} -> the cases, one per signature, in a fixed order"""
    return [c for _, c in sorted(cands.values(), key=lambda sc: (sc[1]["id"]))]


@functools.lru_cache(maxsize=None)
def product_candidates():
    """every (option set, candidate shape) whose plan is launched: [(option set, case, plan record)]"""
    out = []
    for oname, env in OPTION_SETS.items():
        shapes = []
        for kind in KINDS:
            for N in PARTICLES:
                for F in DENSITIES:
                    lo = 1 if (kind in MANIS and F == 2) else 2  # (two: a mixed batch, or one with a two-density product beside F >= 3)
                    for n in (lo,) + PRODUCTS:
                        shapes.append((kind, N, n, F))
        with options(env):
            recs = abi.plan_products([product_query(*s) for s in shapes])
        for (kind, N, n, F), r in zip(shapes, recs):
            if r.status == 0:
                case = {"id": f"{kind}_N{N}_n{n}_F{F}_{oname}", "kind": kind, "N": N, "n": n, "F": F, "options": oname,
                        "plan": r.as_dict(), "sig": product_signature(r)}
                out.append((oname, case, product_signature(r)))
    return out


# Launches that ran past their LDS until the sweep of tests/test_launch_plans.py found them: big plans under
# NBP_PRODUCT_HL2_MIN <= 16 stayed at two helper lanes, on kernels without the scratch path.  Their signatures are those of
# default-option cases, so they stand here by name: (kind, N, n, F, option set).
BIG_UNDER_HL2_MIN = (("e2", 64, 2, 40, "hl2min1"), ("se", 300, 2, 4, "hl2min1"), ("mixed", 300, 17, 4, "hl2min1"))


@functools.lru_cache(maxsize=None)
def product_cases():
    best = {}
    for _, case, sig in product_candidates():
        # (ties: the default options first, then the fewer densities)
        size = (case["N"] * case["n"], case["options"] != "defaults", case["N"] * case["n"] * case["F"], case["id"])
        if sig not in best or size < best[sig][0]:
            best[sig] = (size, case)
    cases = _smallest(best)
    by_id = {case["id"]: case for _, case, _ in product_candidates()}
    for kind, N, n, F, oname in BIG_UNDER_HL2_MIN:
        case = by_id[f"{kind}_N{N}_n{n}_F{F}_{oname}"]
        if case not in cases:
            cases.append(case)
    return cases


@functools.lru_cache(maxsize=None)
def fit_cases():
    """plain launches (run_bandwidth of `n` beliefs on Euclid(2)) and prep launches: the KD builds of one product batch of `n`
    Euclid(2) products of two densities ("prep": an immediate batch has no pending fits beside them) and of a program's round of
    `n` updates, with the fits of its 2 n proposals ("round")"""
    best = {}
    D = abi.MANIFOLD_DIM[FIT_MANIFOLD]
    for oname, env in FIT_OPTION_SETS.items():
        shapes = [("plain", N, k) for N in PARTICLES for k in FITS] + [("prep", N, k) for N in PARTICLES for k in (1,) + FITS] + \
                 [("round", N, k) for N in PARTICLES for k in ROUNDS]
        query = {"plain": lambda N, k: (N, k, k * D, 0, 0, 0), "prep": lambda N, k: (N, 0, 0, k, 2, 0), "round": lambda N, k: (N, 2 * k, 2 * k * D, k, 2, 0)}
        with options(env):
            recs = abi.plan_fits([query[what](N, k) for what, N, k in shapes])
        for (what, N, k), r in zip(shapes, recs):
            case = {"id": f"{what}_N{N}_n{k}_{oname}", "what": what, "N": N, "n": k, "options": oname, "plan": r.as_dict()}
            size = (N * k, case["id"])
            sig = fit_signature(r)
            if sig not in best or size < best[sig][0]:
                best[sig] = (size, case)
    return _smallest(best)
