"""ctypes mirror of include/nbp.h -- the C ABI of libnbp.

The structures here are byte-for-byte the ones declared in ``include/nbp.h``; the same
descriptors are consumed by the HIP library (product) and, in tests only, by the CPU oracle.
"""
import ctypes as C
import os

MAXV, MAXF, MAXD, MAXC, MAXN, COMP_STRIDE = 6, 128, 3, 4, 512, 13

# enum nbp_manifold
EUCLID1, EUCLID2, EUCLID3, CIRCULAR, SE2 = 1, 2, 3, 4, 5
# enum nbp_factor
F_PRIOR, F_MSGPRIOR, F_LINREL, F_CIRCULAR, F_SE2, F_EUCLIDDIST, F_PASSTHROUGH = 1, 2, 3, 4, 5, 6, 7
DIST_GAUSSIAN, DIST_UNIFORM, DIST_RAYLEIGH, DIST_TABLE = 0, 1, 2, 3  # enum nbp_dist: family of a scalar measurement component (comp[c][12])
STAGE_PROPOSALS, STAGE_PRODUCTS, STAGE_COPIES, STAGE_DECONV, STAGE_COPY_POINTS = 1, 2, 3, 4, 5
OPT_LAZY_BANDWIDTH = 1
OPT_GRAPH_REPLAY = 2
OPT_FUSED_UPDATES = 3
OPT_ASYNC_UPLOAD = 4
OPT_UP_PASS_SINKS = 5  # set by nbp_tree_compile for whole-tree programs of one rank; the Python host does not set it

MANIFOLD_DIM = {EUCLID1: 1, EUCLID2: 2, EUCLID3: 3, CIRCULAR: 1, SE2: 3}
MANIFOLD_P = {EUCLID1: 1, EUCLID2: 2, EUCLID3: 3, CIRCULAR: 1, SE2: 6}


class ProposalDesc(C.Structure):
    _fields_ = [
        ("factor_kind", C.c_int32),
        ("manifold", C.c_int32),
        ("nvars", C.c_int32),
        ("sfidx", C.c_int32),
        ("var_slot", C.c_int32 * MAXV),
        ("out_slot", C.c_int32),
        ("ncomp", C.c_int32),
        ("has_multihypo", C.c_int32),
        ("inflate_cycles", C.c_int32),
        ("mhidx_in", C.c_int32),
        ("mhidx_out", C.c_int32),
        ("skip_bandwidth", C.c_int32),
        ("partial_mask", C.c_int32),
        ("meas_kde", C.c_int32),
        ("keep_count", C.c_int32),
        ("multihypo", C.c_double * MAXV),
        ("nullhypo", C.c_double),
        ("inflation", C.c_double),
        ("spread_nh", C.c_double),
        ("comp", (C.c_double * COMP_STRIDE) * MAXC),
        ("seed", C.c_uint64),
        ("meas_seed", C.c_uint64),
    ]


class ProductDesc(C.Structure):
    _fields_ = [
        ("manifold", C.c_int32),
        ("nfactors", C.c_int32),
        ("niter", C.c_int32),
        ("out_slot", C.c_int32),
        ("in_slot", C.c_int32 * MAXF),
        ("labels_out", C.c_int32),
        ("old_slot", C.c_int32),
        ("in_partial", C.c_uint8 * MAXF),
        ("seed", C.c_uint64),
    ]


class CopyDesc(C.Structure):
    _fields_ = [("src_slot", C.c_int32), ("dst_slot", C.c_int32)]


class GridDesc(C.Structure):
    """nbp_grid_desc: one marginal grid of one resident belief (coordinates 0-based; dims[1] = -1: a 1-D grid)"""
    _fields_ = [
        ("slot", C.c_int32),
        ("manifold", C.c_int32),
        ("dims", C.c_int32 * 2),
        ("n", C.c_int32 * 2),
        ("flags", C.c_int32),
        ("lo", C.c_double * 2),
        ("step", C.c_double * 2),
        ("margin", C.c_double),
    ]


GRID_MAX, GRID_AUTO_EXTENT = 1024, 1


class ModesOpts(C.Structure):
    """nbp_modes_opts: the options of the mode finder (the defaults: NBP_MODES_* of include/nbp.h)"""
    _fields_ = [("bw_scale", C.c_double), ("tol", C.c_double), ("merge", C.c_double), ("max_iter", C.c_int32), ("pad", C.c_int32)]


class ModeRec(C.Structure):
    """nbp_mode_rec: one mode of one belief"""
    _fields_ = [("location", C.c_double * MAXD), ("density", C.c_double), ("count", C.c_int32), ("leader", C.c_int32)]


MODES_MAX = 32
MODES_BW_SCALE, MODES_TOL, MODES_MAX_ITER, MODES_MERGE = 2.0, 1e-6, 500, 1e-2

MIX_MAX = 8  # NBP_MIX_MAX: components per nbp_run_mixture
MIX_TOL, MIX_MAX_ITER = 1e-8, 500


class MixtureOpts(C.Structure):
    """nbp_mixture_opts: the stopping rule of the mixture fit (the defaults: NBP_MIX_* of include/nbp.h)"""
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int32), ("pad", C.c_int32)]


class MixtureRec(C.Structure):
    """nbp_mixture_rec: one belief of nbp_run_mixture, the components by weight descending; entries from n_comp on are zero"""
    _fields_ = [("weight", C.c_double * MIX_MAX), ("mean", (C.c_double * MAXD) * MIX_MAX), ("cov", (C.c_double * (MAXD * MAXD)) * MIX_MAX),
                ("objective", C.c_double), ("count", C.c_int32 * MIX_MAX), ("n_comp", C.c_int32), ("iters", C.c_int32),
                ("converged", C.c_int32), ("n_dropped", C.c_int32)]


class LikelihoodDesc(C.Structure):
    """nbp_likelihood_desc: one item of nbp_run_factor_likelihood -- a measurement model and the slots of its one or two roles"""
    _fields_ = [("kind", C.c_int32), ("manifold", C.c_int32), ("slot_a", C.c_int32), ("slot_b", C.c_int32), ("ncomp", C.c_int32),
                ("partial_mask", C.c_int32), ("comp", (C.c_double * COMP_STRIDE) * MAXC)]


class ProductItem(C.Structure):
    """nbp_product_item: one message of nbp_run_product_grid -- a measurement model (its own slots are not read), the role the grid's
    variable fills (0: a, 1: b), the slot of the other variable (-1: unary), the group (a multihypo factor) and the log prior"""
    _fields_ = [("lik", LikelihoodDesc), ("role", C.c_int32), ("other", C.c_int32), ("group", C.c_int32), ("pad", C.c_int32),
                ("log_prior", C.c_double)]


class ProductGridDesc(C.Structure):
    """nbp_product_grid_desc: one grid over all coordinates of a variable (flags & PGRID_AUTO_EXTENT: lo and step are not read, the
    belief in `slot` is) and the range of items it multiplies"""
    _fields_ = [("manifold", C.c_int32), ("slot", C.c_int32), ("n", C.c_int32 * 3), ("flags", C.c_int32), ("first_item", C.c_int32),
                ("n_items", C.c_int32), ("lo", C.c_double * 3), ("step", C.c_double * 3), ("margin", C.c_double)]


class ProductGridRec(C.Structure):
    """nbp_product_grid_rec"""
    _fields_ = [("logZ", C.c_double), ("logmax", C.c_double), ("argmax", C.c_int32), ("pad", C.c_int32)]


PGRID_AUTO_EXTENT, PGRID_MAX_CELLS, PGRID_CHUNK, PGRID_MARGIN = 1, 1 << 22, 256, 4.0


MAXK = 8  # NBP_MAXK: groups (modes) per belief in nbp_run_factor_mode_likelihood


class OverlapRec(C.Structure):
    """nbp_overlap_rec: one pair of nbp_run_overlap -- logc = lab - (laa + lbb) / 2"""
    _fields_ = [("logc", C.c_double), ("lab", C.c_double), ("laa", C.c_double), ("lbb", C.c_double)]


class OverlapOpts(C.Structure):
    """nbp_overlap_opts: the options of the overlap search (the defaults: NBP_OVERLAP_* of include/nbp.h)"""
    _fields_ = [("reach", C.c_double), ("min_coeff", C.c_double), ("topk", C.c_int32), ("pad", C.c_int32)]


OVERLAP_MAXK, OVERLAP_REACH, OVERLAP_MIN_COEFF, OVERLAP_TOPK = 16, 6.0, 1e-3, 8


class SceneDesc(C.Structure):
    """nbp_scene_desc: the one grid of nbp_run_scene_grid (flags & SCENE_AUTO_EXTENT: lo and step are not read)"""
    _fields_ = [("n", C.c_int32 * 2), ("flags", C.c_int32), ("pad", C.c_int32), ("lo", C.c_double * 2), ("step", C.c_double * 2),
                ("margin", C.c_double), ("reach", C.c_double)]


SCENE_AUTO_EXTENT, SCENE_MAX, SCENE_REACH, SCENE_MARGIN, SCENE_MAX_POINTS = 1, 4096, 6.0, 4.0, 1 << 22

CRED_MAX = 8  # NBP_CRED_MAX: masses and probabilities per nbp_run_credible


class CredibleOpts(C.Structure):
    """nbp_credible_opts: the masses of the HDR levels and the probabilities of the coordinate quantiles"""
    _fields_ = [("n_mass", C.c_int32), ("n_prob", C.c_int32), ("mass", C.c_double * CRED_MAX), ("prob", C.c_double * CRED_MAX)]


class CredibleRec(C.Structure):
    """nbp_credible_rec: one belief of nbp_run_credible; unused entries are zero"""
    _fields_ = [("log_level", C.c_double * CRED_MAX), ("quant", (C.c_double * CRED_MAX) * MAXD), ("mean", C.c_double * MAXD),
                ("log_min", C.c_double), ("log_max", C.c_double), ("n_inside", C.c_int32 * CRED_MAX), ("count", C.c_int32),
                ("pad", C.c_int32)]


class CredibilityRec(C.Structure):
    """nbp_credibility_rec: one query of nbp_run_credible -- mass = n_above / count"""
    _fields_ = [("logdens", C.c_double), ("mass", C.c_double), ("n_above", C.c_int32), ("pad", C.c_int32)]


ERR_INVALID = -5  # NBP_ERR_INVALID: what the heatmap entry points refuse
HM_MAX_CELLS = 1 << 26


class Xfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("slot", C.c_int32)]


COMM_ID_BYTES = 128


class Diag(C.Structure):
    _fields_ = [
        ("solves", C.c_int64),
        ("nonconverged", C.c_int64),
        ("nan_results", C.c_int64),
        ("residual_evals", C.c_int64),
        ("lcv_evals", C.c_int64),
        ("lcv_evals_f32", C.c_int64),
        ("proposal_launches_workgroup", C.c_int64),
        ("proposal_launches_wave", C.c_int64),
        ("proposal_launches_split", C.c_int64),
        ("lane_side_launches", C.c_int64),
        ("lane_waits", C.c_int64),
        ("lane_side_updates", C.c_int64),
        ("sunk_updates", C.c_int64),
        ("sink_launches", C.c_int64),
    ]


class LanePartRec(C.Structure):
    """nbp_lane_part_rec: one part of a program with lanes (nbp_program_lane_plan)"""
    _fields_ = [("stage", C.c_int32), ("lane", C.c_int32), ("first_desc", C.c_int32), ("n", C.c_int32), ("wait", C.c_int32), ("signals", C.c_int32)]


class ProductPlanReq(C.Structure):
    """nbp_product_plan_req: one product launch as nbp_plan_products takes it"""
    _fields_ = [(k, C.c_int32) for k in ("N", "n", "F", "D", "mani", "geom_n")]


PLAN_REFUSED_BIG_IN_ROUND, PLAN_REFUSED_LDS, PLAN_REFUSED_NO_KERNEL = 1, 2, 3


class _PlanRec(C.Structure):
    def as_dict(self):
        return {k: (getattr(self, k).decode() if k == "kernel" else getattr(self, k)) for k, _ in self._fields_ if not k.startswith("pad")}


class ProductPlanRec(_PlanRec):
    """nbp_product_plan_rec: what a product launch runs (nbp_plan_products, nbp_last_plans)"""
    _fields_ = [(k, C.c_int32) for k in ("status", "refusal", "HL", "wpb", "G", "big", "xs", "circ", "nch", "all_levels", "w1", "row", "row_HL",
                                         "row_mani", "row_xs", "row_w1", "launch_bound", "N", "n", "F", "D", "mani", "geom_n", "pad")] + \
               [("lds", C.c_int64), ("gstats", C.c_int64), ("kernel", C.c_char * 40)]


class FitPlanReq(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("N", "fits", "coords", "products", "kdF", "geom_blocks")]


class FitPlanRec(_PlanRec):
    _fields_ = [(k, C.c_int32) for k in ("status", "P", "depth", "KS", "w5", "threads", "prep", "kd_nostats", "N", "fits", "coords", "products",
                                         "kdF", "geom_blocks")] + [("pad", C.c_int32 * 2), ("lds", C.c_int64), ("kernel", C.c_char * 40)]


class ProposalPlanReq(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("N", "n", "manifold", "simple")]


class ProposalPlanRec(_PlanRec):
    _fields_ = [(k, C.c_int32) for k in ("status", "geometry", "blocks", "threads", "N", "n", "manifold", "simple")] + \
               [("lds", C.c_int64), ("kernel", C.c_char * 40)]


def _plan(fn_name, Req, Rec, reqs):
    """the batched plan queries: a list of tuples in the field order of `Req` -> a ctypes array of `Rec` (no context, no GPU)"""
    lib = load_library()
    n = len(reqs)
    arr = (Req * n)(*[Req(*r) for r in reqs])
    out = (Rec * n)()
    rc = getattr(lib, fn_name)(arr, out, n)
    if rc != 0:
        raise ValueError(f"{fn_name}: status {rc}: {lib.nbp_last_error().decode()}")
    return out


def plan_products(reqs):
    """reqs: (N, n, F, D, mani, geom_n) each -> ProductPlanRec array"""
    return _plan("nbp_plan_products", ProductPlanReq, ProductPlanRec, reqs)


def plan_fits(reqs):
    """reqs: (N, fits, coords, products, kdF, geom_blocks) each -> FitPlanRec array"""
    return _plan("nbp_plan_fits", FitPlanReq, FitPlanRec, reqs)


def plan_proposals(reqs):
    """reqs: (N, n, manifold, simple) each -> ProposalPlanRec array"""
    return _plan("nbp_plan_proposals", ProposalPlanReq, ProposalPlanRec, reqs)


def slot_stride(N):
    return 3 * N + 8


_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "csrc", "libnbp.so")

# every symbol include/nbp.h declares (tests check the .so exports all of them)
EXPORTS = [
    "nbp_arena_bytes", "nbp_slot_stride_doubles", "nbp_ctx_create", "nbp_ctx_destroy",
    "nbp_last_error", "nbp_synchronize", "nbp_arena_ptr", "nbp_stream_ptr", "nbp_ctx_particles", "nbp_ctx_slots", "nbp_ctx_device",
    "nbp_ctx_reserve_resident", "nbp_ctx_resident", "nbp_belief_write_batch_async", "nbp_belief_read_batch_begin", "nbp_belief_read_batch_end",
    "nbp_run_copies_async", "nbp_program_retire",
    "nbp_slot_write", "nbp_slot_read", "nbp_belief_write", "nbp_belief_read", "nbp_belief_write_batch", "nbp_belief_read_batch", "nbp_run_resample", "nbp_side_write", "nbp_side_read",
    "nbp_run_proposals", "nbp_run_bandwidth", "nbp_run_ppe", "nbp_kde_ppe", "nbp_run_evaluate", "nbp_kde_evaluate", "nbp_run_marginal_grid", "nbp_kde_marginal_grid", "nbp_run_evaluate_marginal", "nbp_run_mmd", "nbp_kde_mmd", "nbp_run_meancov", "nbp_kde_meancov", "nbp_run_kld", "nbp_kde_kld", "nbp_run_overlap", "nbp_kde_overlap", "nbp_run_overlap_search", "nbp_run_scene_grid", "nbp_run_credible", "nbp_kde_credible", "nbp_run_modes", "nbp_kde_modes", "nbp_run_mixture", "nbp_kde_mixture", "nbp_run_factor_likelihood", "nbp_factor_likelihood", "nbp_run_factor_mode_likelihood", "nbp_factor_mode_likelihood", "nbp_run_product_grid", "nbp_product_grid", "nbp_heatmap_create", "nbp_heatmap_build", "nbp_heatmap_draw", "nbp_heatmap_info", "nbp_heatmap_destroy", "nbp_heatmap_scan_eval", "nbp_heatmap_search_eval", "nbp_run_products", "nbp_run_copies", "nbp_run_deconv", "nbp_kde_bandwidth", "nbp_conv", "nbp_manifold_product",
    "nbp_program_create", "nbp_program_add_stage", "nbp_program_set_option", "nbp_program_finalize", "nbp_program_run",
    "nbp_program_reseed", "nbp_program_num_seeds", "nbp_program_set_seeds", "nbp_program_seed_order", "nbp_ctx_attach", "nbp_ctx_attached", "nbp_program_num_stages", "nbp_program_num_fused", "nbp_program_num_two_stream", "nbp_program_set_lanes", "nbp_program_lane_plan", "nbp_program_sink_plan", "nbp_program_destroy",
    "nbp_timing_enable", "nbp_timing_read", "nbp_timing_read_n", "nbp_diag_read",
    "nbp_plan_products", "nbp_plan_fits", "nbp_plan_proposals", "nbp_last_plans",
    "nbp_comm_unique_id", "nbp_comm_create", "nbp_comm_destroy", "nbp_comm_info", "nbp_exchange", "nbp_math_eval",
]

_lib = None


def load_library(path=None):
    """dlopen libnbp.so and declare argument types.  Fails loudly when the HIP extension has
    not been built -- there is no CPU fallback in the product path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("NBP_LIB_OVERRIDE") or LIB_PATH  # override: kernel experiments (tools/exp)
    if not os.path.exists(path):
        raise RuntimeError(
            f"libnbp.so not found at {path}: build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950). The product path has no CPU fallback."
        )
    # One HIP runtime per process.  PyTorch ships its own libamdhip64 / libhsa-runtime64 with the same
    # SONAMEs as /opt/rocm; if libnbp pulled in the system copies first, a later `import torch` (the
    # multi-GPU path: torch-owned arena + torch.distributed) would bring up a second runtime that cannot
    # open the GPU ("No HIP GPUs are available").  Importing torch first makes libnbp bind to the copies
    # torch loaded.  Without PyTorch (e.g. the Julia shim) the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    lib.nbp_arena_bytes.restype = i64
    lib.nbp_arena_bytes.argtypes = [i32, i32]
    lib.nbp_slot_stride_doubles.restype = i64
    lib.nbp_slot_stride_doubles.argtypes = [i32]
    lib.nbp_ctx_create.argtypes = [i32, i32, i32, vp, i64, i32, C.POINTER(vp)]
    lib.nbp_ctx_destroy.argtypes = [vp]
    lib.nbp_last_error.restype = C.c_char_p
    lib.nbp_synchronize.argtypes = [vp]
    lib.nbp_arena_ptr.restype = vp
    lib.nbp_arena_ptr.argtypes = [vp]
    lib.nbp_stream_ptr.restype = vp
    lib.nbp_stream_ptr.argtypes = [vp]
    lib.nbp_ctx_particles.argtypes = [vp]
    lib.nbp_ctx_slots.argtypes = [vp]
    lib.nbp_ctx_device.argtypes = [vp]
    lib.nbp_slot_write.argtypes = [vp, i32, i32, dp, dp]
    lib.nbp_slot_read.argtypes = [vp, i32, i32, dp, dp]
    lib.nbp_belief_write.argtypes = [vp, i32, i32, dp, i32, dp, dp]
    lib.nbp_belief_read.argtypes = [vp, i32, i32, dp, ip, dp, dp]
    lib.nbp_belief_write_batch.argtypes = [vp, i32, ip, ip, C.POINTER(dp), ip, C.POINTER(dp), C.POINTER(dp)]
    lib.nbp_belief_read_batch.argtypes = [vp, i32, ip, ip, C.POINTER(dp), ip, C.POINTER(dp), C.POINTER(dp)]
    lib.nbp_run_resample.argtypes = [vp, ip, ip, i32, C.c_uint64]
    lib.nbp_side_write.argtypes = [vp, i32, ip, i32]
    lib.nbp_side_read.argtypes = [vp, i32, ip, i32]
    lib.nbp_run_proposals.argtypes = [vp, C.POINTER(ProposalDesc), i32]
    lib.nbp_run_bandwidth.argtypes = [vp, ip, ip, i32]
    lib.nbp_run_ppe.argtypes = [vp, ip, ip, i32, dp, dp, ip]
    lib.nbp_kde_ppe.argtypes = [vp, i32, dp, i32, dp, dp, dp, ip]
    lib.nbp_run_evaluate.argtypes = [vp, ip, ip, i32, ip, dp, dp]
    lib.nbp_kde_evaluate.argtypes = [vp, i32, dp, i32, dp, dp, i32, dp]
    lib.nbp_run_marginal_grid.argtypes = [vp, C.POINTER(GridDesc), i32, ip, dp, dp]
    lib.nbp_kde_marginal_grid.argtypes = [vp, i32, dp, i32, dp, C.POINTER(GridDesc), dp, dp]
    lib.nbp_run_evaluate_marginal.argtypes = [vp, ip, ip, ip, i32, ip, dp, dp]
    lib.nbp_run_mmd.argtypes = [vp, ip, ip, ip, i32, C.c_double, dp]
    lib.nbp_kde_mmd.argtypes = [vp, i32, dp, i32, dp, i32, C.c_double, dp]
    lib.nbp_run_meancov.argtypes = [vp, ip, ip, i32, dp, dp]
    lib.nbp_kde_meancov.argtypes = [vp, i32, dp, i32, dp, dp]
    lib.nbp_run_kld.argtypes = [vp, ip, ip, ip, i32, dp, dp]
    lib.nbp_kde_kld.argtypes = [vp, i32, dp, i32, dp, dp, i32, dp, dp, dp]
    lib.nbp_run_overlap.argtypes = [vp, ip, ip, ip, ip, ip, ip, i32, C.POINTER(OverlapRec)]
    lib.nbp_kde_overlap.argtypes = [vp, i32, dp, i32, dp, i32, i32, dp, i32, dp, i32, C.POINTER(OverlapRec)]
    lib.nbp_run_overlap_search.argtypes = [vp, ip, ip, ip, i32, C.POINTER(OverlapOpts), ip, dp, ip, ip]
    lib.nbp_run_scene_grid.argtypes = [vp, ip, ip, ip, dp, i32, C.POINTER(SceneDesc), dp, ip, ip, dp, C.POINTER(i64)]
    lib.nbp_run_credible.argtypes = [vp, ip, ip, ip, i32, C.POINTER(CredibleOpts), ip, dp, C.POINTER(CredibleRec), dp, ip,
                                     C.POINTER(CredibilityRec)]
    lib.nbp_kde_credible.argtypes = [vp, i32, dp, i32, dp, i32, C.POINTER(CredibleOpts), dp, i32, C.POINTER(CredibleRec), dp, ip,
                                     C.POINTER(CredibilityRec)]
    lib.nbp_run_modes.argtypes = [vp, ip, ip, i32, C.POINTER(ModesOpts), C.POINTER(ModeRec), ip, ip, ip, ip]
    lib.nbp_kde_modes.argtypes = [vp, i32, dp, i32, dp, C.POINTER(ModesOpts), C.POINTER(ModeRec), ip, ip, ip, ip]
    lib.nbp_run_mixture.argtypes = [vp, ip, ip, i32, ip, ip, dp, C.POINTER(MixtureOpts), C.POINTER(MixtureRec), ip]
    lib.nbp_kde_mixture.argtypes = [vp, i32, dp, i32, dp, ip, dp, C.POINTER(MixtureOpts), C.POINTER(MixtureRec), ip]
    lib.nbp_run_factor_likelihood.argtypes = [vp, C.POINTER(LikelihoodDesc), i32, dp, dp]
    lib.nbp_factor_likelihood.argtypes = [vp, C.POINTER(LikelihoodDesc), dp, i32, dp, i32, dp, dp]
    lib.nbp_run_factor_mode_likelihood.argtypes = [vp, C.POINTER(LikelihoodDesc), ip, ip, i32, ip, i32, dp, ip]
    lib.nbp_factor_mode_likelihood.argtypes = [vp, C.POINTER(LikelihoodDesc), dp, i32, ip, dp, i32, ip, dp, ip]
    lib.nbp_run_product_grid.argtypes = [vp, C.POINTER(ProductGridDesc), i32, C.POINTER(ProductItem), i32, ip, dp, C.POINTER(ProductGridRec), dp]
    lib.nbp_product_grid.argtypes = [vp, C.POINTER(ProductGridDesc), C.POINTER(ProductItem), i32, C.POINTER(dp), ip, dp, i32, dp, dp,
                                     C.POINTER(ProductGridRec), dp]
    lib.nbp_heatmap_create.argtypes = [vp, dp, i32, i32, dp, dp, C.c_double, C.POINTER(vp)]
    lib.nbp_heatmap_build.argtypes = [vp, i32, C.c_uint64, ip, dp, dp, dp]
    lib.nbp_heatmap_draw.argtypes = [vp, i32, C.c_uint64, i32, i32, ip, dp, dp]
    lib.nbp_heatmap_info.argtypes = [vp, dp, dp, dp, ip]
    lib.nbp_heatmap_destroy.argtypes = [vp]
    lib.nbp_heatmap_scan_eval.argtypes = [vp, dp, i32, dp]
    lib.nbp_heatmap_search_eval.argtypes = [vp, dp, i32, dp, i32, ip]
    lib.nbp_run_deconv.argtypes = [vp, C.POINTER(ProposalDesc), ip, i32]
    dpp = C.POINTER(dp)
    lib.nbp_kde_bandwidth.argtypes = [vp, i32, dp, dp]
    lib.nbp_conv.argtypes = [vp, C.POINTER(ProposalDesc), dpp, dpp, ip, dp, dp, ip]
    lib.nbp_manifold_product.argtypes = [vp, i32, i32, dpp, dpp, C.POINTER(C.c_uint8), dp, i32, C.c_uint64, dp, dp, ip]
    lib.nbp_run_products.argtypes = [vp, C.POINTER(ProductDesc), i32]
    lib.nbp_run_copies.argtypes = [vp, C.POINTER(CopyDesc), i32]
    lib.nbp_program_create.argtypes = [vp, C.POINTER(vp)]
    lib.nbp_program_add_stage.argtypes = [vp, i32, vp, i32]
    lib.nbp_program_set_option.argtypes = [vp, i32, i32]
    lib.nbp_program_finalize.argtypes = [vp]
    lib.nbp_program_run.argtypes = [vp, i32, i32]
    lib.nbp_program_reseed.argtypes = [vp, C.c_uint64]
    lib.nbp_program_num_seeds.argtypes = [vp, ip]
    lib.nbp_program_set_seeds.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    lib.nbp_program_seed_order.argtypes = [vp, ip, i32]
    lib.nbp_program_num_stages.argtypes = [vp, ip]
    lib.nbp_program_destroy.argtypes = [vp]
    lib.nbp_comm_unique_id.argtypes = [vp]
    lib.nbp_comm_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    lib.nbp_comm_destroy.argtypes = [vp]
    lib.nbp_comm_info.argtypes = [vp, ip, ip]
    lib.nbp_math_eval.argtypes = [vp, i32, dp, dp, dp, dp, i64]
    lib.nbp_exchange.argtypes = [vp, vp, C.POINTER(Xfer), i32, C.POINTER(Xfer), i32]
    lib.nbp_timing_enable.argtypes = [vp, i32]
    lib.nbp_timing_read.argtypes = [vp, dp, C.POINTER(i64)]
    lib.nbp_timing_read_n.argtypes = [vp, dp, C.POINTER(i64), i32]
    lib.nbp_program_num_fused.argtypes = [vp, C.POINTER(i32)]
    lib.nbp_program_num_two_stream.argtypes = [vp, C.POINTER(i32)]
    lib.nbp_program_set_lanes.argtypes = [vp, i32, ip, i32]
    lib.nbp_program_lane_plan.argtypes = [vp, C.POINTER(LanePartRec), i32, C.POINTER(i32)]
    lib.nbp_program_sink_plan.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.nbp_diag_read.argtypes = [vp, C.POINTER(Diag), i32]
    lib.nbp_plan_products.argtypes = [C.POINTER(ProductPlanReq), C.POINTER(ProductPlanRec), i64]
    lib.nbp_plan_fits.argtypes = [C.POINTER(FitPlanReq), C.POINTER(FitPlanRec), i64]
    lib.nbp_plan_proposals.argtypes = [C.POINTER(ProposalPlanReq), C.POINTER(ProposalPlanRec), i64]
    lib.nbp_last_plans.argtypes = [vp, C.POINTER(ProductPlanRec), C.POINTER(FitPlanRec), C.POINTER(FitPlanRec)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int32
    if path == LIB_PATH:
        _lib = lib
    return lib
