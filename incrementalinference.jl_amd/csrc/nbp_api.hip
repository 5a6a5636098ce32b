// nbp_api.hip -- host side of libnbp: the C ABI declared in include/nbp.h.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC nbp_api.hip -o libnbp.so
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <unordered_map>

#include <dlfcn.h>
#include <algorithm>
#include <rccl/rccl.h>  // types and prototypes only: the entry points are resolved with dlsym (see rccl_api)

#ifndef NBP_TU
#define NBP_TU 0  // host code: the kernels live in the nbp_k_*.hip files (-DNBP_TU=NBP_TU_ALL: single-file build with every kernel)
#endif
#include "nbp_kernels.h"
#include "nbp_fused.h"
#include "nbp_ppe.h"
#include "nbp_query.h"
#include "nbp_stats.h"
#include "nbp_marginal.h"
#include "nbp_heatmap.h"
#include "nbp_modes.h"
#include "nbp_likelihood.h"
#include "nbp_overlap.h"
#include "nbp_credible.h"
#include "nbp_mixture.h"
#include "nbp_scene.h"
#include "nbp_productgrid.h"
#include "../../include/nbp_lanes.h"
#include "../../include/nbp_sinks.h"

static thread_local std::string g_err;
static nbp_status fail(nbp_status code, const std::string &msg) {
  g_err = msg;
  return code;
}
// shared with nbp_host.cpp (same library): sets the message nbp_last_error() returns
// host-side loops over many beliefs (a tree level's worth of them packed into / unpacked from the staging buffer, ~1 us
// each): a few threads when there is enough work (profiles/r04_clique_seam_phases.txt)
template <class F>
static void host_parallel_for(int n, int grain, F &&f) {
  const unsigned hw = std::thread::hardware_concurrency();
  int nt = n / grain;
  if (nt > 8) nt = 8;
  if (hw && nt > (int)hw) nt = (int)hw;
  if (nt <= 1) {
    for (int i = 0; i < n; i++) f(i);
    return;
  }
  auto part = [&](int t) {
    const int a = (int)((int64_t)n * t / nt), b = (int)((int64_t)n * (t + 1) / nt);
    for (int i = a; i < b; i++) f(i);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(part, t);
  part(0);
  for (std::thread &x : th) x.join();
}

extern "C" nbp_status nbp_internal_fail(nbp_status code, const char *msg) { return fail(code, msg ? msg : ""); }
#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(NBP_ERR_HIP, std::string(#expr) + " (nbp_api.hip:" + std::to_string(__LINE__) + "): " + hipGetErrorString(e_)); \
  } while (0)

// Speculative fits (lcv_bandwidth_1d_spec): used when every workgroup of the launch is resident at once -- the launch,
// with 3 or 7 workgroups per fitted coordinate, stays below NBP_SPEC_MAXBLOCKS (the chip has 256 CUs and a fit's
// workgroup has a CU to itself: 1024 lanes, ~63 KB of LDS).  Counted are the workgroups that stay: those of a
// coordinate the manifold does not have leave at once (`coords` = sum of the manifold dimensions of the jobs).
#ifndef NBP_SPEC_MAXJOBS
#define NBP_SPEC_MAXJOBS 40
#endif
#ifndef NBP_SPEC_MAXBLOCKS
#define NBP_SPEC_MAXBLOCKS 224
#endif
struct nbp_program;
struct nbp_comm;
struct nbp_ctx {
  std::vector<nbp_heatmap *> heatmaps;  // live heatmap densities: their device memory is freed (ctx = null) by nbp_ctx_destroy
  std::vector<nbp_program *> programs;  // live programs: detached (device blob freed, ctx = null) by nbp_ctx_destroy
  std::vector<nbp_comm *> comms;        // live communicators: shut down (and detached) by nbp_ctx_destroy
  void *attached = nullptr;             // an object of the layer above (nbp_ctx_attach: the native host's plan cache) ...
  void (*attached_destroy)(void *) = nullptr;  // ... destroyed at the top of nbp_ctx_destroy, while the context is whole
  uint64_t ws_gen = 0;  // bumped whenever a workspace a captured launch sequence holds by value (ws, gstats) is re-allocated
  int device = 0, N = 0, n_slots = 0, side_ints = 0, threads = 0, Npad = 0, P = 1;
  int64_t S = 0;
  double *arena = nullptr;
  bool own_arena = false;
  int32_t *side = nullptr;
  nbp_counters *counters = nullptr;
  hipStream_t stream = nullptr;
  nbp_levels T{};
  int32_t *lv_ints = nullptr;
  double *lv_dbls = nullptr;
  double *ws = nullptr;  // KD workspace: [products][kdF] x nbp_kd_ws_doubles(N), kdF = largest F of the batch
  size_t ws_doubles = 0;
  nbp_spec_area *spec = nullptr;  // rendezvous areas of the speculative fits (latency-mode launches), NBP_SPEC_MAXJOBS x 3
  bool spec_on = true;
  bool spec_depth3 = true;  // 7 workgroups per fit (three iterations per rendezvous) where the launch still fits the chip; NBP_SPEC_DEPTH3=0: 3 only
  double *gstats = nullptr;  // node statistics of products too large for the LDS
  size_t gstats_doubles = 0;
  // staging for immediate-mode calls
  void *stage = nullptr;
  size_t stage_bytes = 0;
  // point estimates, belief queries and statistics (nbp_run_ppe / nbp_run_evaluate / nbp_run_mmd / nbp_run_meancov / nbp_run_kld /
  // nbp_run_marginal_grid): the queries going in and the values or records coming out, grown on demand
  double *query = nullptr;
  size_t query_cap = 0;
  // pinned host staging of the batched belief transfers (nbp_belief_write_batch / _read_batch): one copy per run of
  // consecutive slots, asynchronous on the library stream
  double *pin = nullptr;
  size_t pin_doubles = 0;
  // device blobs of destroyed programs, kept for the next short-lived one (a clique call compiles, runs and drops a
  // program: hipMalloc / hipFree per call would synchronise the whole device each time)
  std::vector<std::pair<char *, size_t>> blob_cache;
  // ---- the asynchronous clique seam (nbp_clique_submit_batch / nbp_clique_wait, nbp_host.h) ----
  // pinned staging buffers of transfers that are queued WITHOUT waiting for the stream: a buffer is free again once the
  // event recorded behind its copy has completed (never waited for: a busy pool grows by a buffer)
  struct pin_buf { char *p = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool pending = false, held = false; };
  std::vector<pin_buf *> pin_pool;
  // programs handed to nbp_program_retire: destroyed once the event recorded behind their last launch has completed
  std::vector<std::pair<nbp_program *, hipEvent_t>> retired;
  int resident = 0;  // the LAST `resident` slots of the arena are resident slots (nbp_ctx_reserve_resident): handle h = slot n_slots - h
  // fused variable updates (nbp_fused.h) for the stages that fill the chip: NBP_NO_FUSED_UPDATE=1 turns them off,
  // NBP_FUSED_MIN = smallest stage (updates) that runs fused
  // Off unless NBP_FUSED_MIN is set: measured on config 2 and on the 10 000-variable chain the fused form moves a ninth of
  // the bytes and takes 10-35 % longer (one workgroup serialises the six fits of an update that the
  // three-launch form spreads over the chip).
  bool fused_on = true;
  int fused_min = 1 << 30;
  // smallest launch of simple Euclidean proposals that runs one WAVE per proposal (launch_proposals); -1: the default of the
  // class (NBP_PROPOSAL_WAVE_MIN overrides it for every class)
  int prop_wave_min = -1;
  // smallest launch of simple Euclid(2) proposals that runs TWO waves per proposal (below it: the workgroup kernel; from
  // prop_wave_min on: the one-wave kernel); -1: the default (NBP_PROPOSAL_SPLIT_MIN overrides it)
  int prop_split_min = -1;
  // launches of launch_proposals by geometry since the last reset of nbp_diag_read: workgroup, one wave, split
  int64_t prop_launches[3] = {0, 0, 0};
  int fused_p1_min = 2048;  // rounds with at least this many updates run one lane per particle (NBP_FUSED_P1_MIN); smaller
                            // ones two helper rows per update, so that they fill the chip with twice the lanes each
  // two-stream rounds (NBP_PIPELINE_MIN = smallest product batch; see plan_pipeline): the second stream and the fork / join
  // events (what a half launches with is its nbp_launch_env)
  hipStream_t stream2 = nullptr;
  hipEvent_t pipe_ev[2] = {nullptr, nullptr};
  int pipe_min = 1 << 30;
  // program lanes (plan_lanes / run_lanes): lane 1 runs on stream2 with a rendezvous area (the second half of `spec`), a
  // statistics area and a share of the KD workspace of its own; the events of the cross-lane waits, per recording lane, plus
  // the fork and the join of a range.  NBP_NO_LANES=1: hints are ignored (the launch sequence of a program without them)
  bool no_lanes = false;
  std::vector<hipEvent_t> lane_ev;  // one per signalling part of the largest program with lanes (presize)
  hipEvent_t lane_fork = nullptr, lane_join = nullptr;
  double *gstats1 = nullptr;
  size_t gstats1_doubles = 0;
  // since the last reset of nbp_diag_read, counted where the launch is issued: launches on lane 1, cross-lane waits, updates
  // (product descriptors) that ran on lane 1
  int64_t lane_side_launches = 0, lane_waits = 0, lane_side_updates = 0;
  // sinks (plan_sinks: NBP_OPT_UP_PASS_SINKS).  NBP_NO_SINKS=1: the option is ignored (A/B runs); NBP_SINK_PLACEMENT=1: one sink
  // per pass, its last step (nbp_sinks.h).  Counted like the lanes': updates that ran in a later stage than their own, and
  // the launches of the parts they ran in
  bool no_sinks = false;
  int sink_placement = 0;
  int64_t sunk_updates = 0, sink_launches = 0;
  // fit launches (fit_plan): NBP_LCV_P2_MIN / NBP_LCV_P1_MIN = workgroups of a launch above which a fit runs on two / one helper
  // rows; NBP_NO_W5_FITS: never the five-wave instances; NBP_DEBUG_OCCUPANCY: print what the runtime says a CU holds of a
  // plain bandwidth launch
  int lcv_p2_min = 256, lcv_p1_min = 4 * 256;
  bool fit_w5 = true, debug_occupancy = false;
  // product launches (product_plan): NBP_PRODUCT_HL2_MIN = smallest batch in the throughput geometry, NBP_PRODUCT_NCH = chunks
  // per helper range (0: as many as the LDS takes), NBP_PRODUCT_ALL_LEVELS_HL = fewest helper lanes that stage every level at
  // once; NBP_NO_XS_PRODUCTS: node sums from the KD workspace only; NBP_NO_UNIFORM_LATENCY_PRODUCTS: the generic latency
  // kernels (for A/B runs and tests)
  int prod_hl2_min = 192, prod_nch = 0, prod_all_levels_hl = 8;
  bool prod_xs = true, prod_lat_uni = true;
  // what the last product / prep / plain bandwidth launch ran (nbp_last_plans): stored on the host where the launch is issued
  nbp_product_plan_rec last_product{};
  nbp_fit_plan_rec last_prep{}, last_fit{};
  // timing: 0 proposal, 1 prep, 2 product, 3 plain bandwidth, 4 fused update kernel
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[5];
  double ms[5] = {0, 0, 0, 0, 0};
  int64_t nl[5] = {0, 0, 0, 0, 0};
};

// The product kernels: helper lanes per sample, the manifold of a single-manifold instance (0: any mix), node sums from the
// sorted coordinates (`xs`), launch bound for at most one workgroup per CU (`w1`).  product_plan picks its kernel here.
typedef void (*nbp_product_fn)(const nbp_product_desc *, double *, const double *, int, double *, int, int64_t, int32_t *, nbp_levels);
struct nbp_product_kernel_row { nbp_product_fn fn; int HL, mani; bool xs, w1; const char *name; int lb; };
// (name and launch bound of a row: the kernel's own, NBP_PRODUCT_LATENCY / NBP_PRODUCT_UNIFORM / NBP_PRODUCT_LATENCY_UNIFORM in nbp_kernels.h)
#define NBP_ROW(NAME, HL_, MANI_, XS_, W1_, LB_) {NAME, HL_, MANI_, XS_, W1_, #NAME, LB_}
static const nbp_product_kernel_row NBP_PRODUCT_KERNELS[] = {
    NBP_ROW(nbp_product_kernel_y32, 32, 0, false, false, 512),           NBP_ROW(nbp_product_kernel_y32_w1, 32, 0, false, true, 256),
    NBP_ROW(nbp_product_kernel_l8, 8, 0, false, false, 512),             NBP_ROW(nbp_product_kernel_l8_w1, 8, 0, false, true, 256),
    NBP_ROW(nbp_product_kernel_t2, 2, 0, false, false, 512),
    NBP_ROW(nbp_product_kernel_y32_e1, 32, NBP_EUCLID1, false, false, 512), NBP_ROW(nbp_product_kernel_y32_e2, 32, NBP_EUCLID2, false, false, 512),
    NBP_ROW(nbp_product_kernel_y32_e3, 32, NBP_EUCLID3, false, false, 512), NBP_ROW(nbp_product_kernel_y32_ci, 32, NBP_CIRCULAR, false, false, 512),
    NBP_ROW(nbp_product_kernel_y32_se, 32, NBP_SE2, false, false, 512),
    NBP_ROW(nbp_product_kernel_l8_e1, 8, NBP_EUCLID1, false, false, 512),   NBP_ROW(nbp_product_kernel_l8_e2, 8, NBP_EUCLID2, false, false, 512),
    NBP_ROW(nbp_product_kernel_l8_e3, 8, NBP_EUCLID3, false, false, 512),   NBP_ROW(nbp_product_kernel_l8_ci, 8, NBP_CIRCULAR, false, false, 512),
    NBP_ROW(nbp_product_kernel_l8_se, 8, NBP_SE2, false, false, 512),
    NBP_ROW(nbp_product_kernel_t2_e1, 2, NBP_EUCLID1, false, false, NBP_PROD_LB(NBP_EUCLID1)),   NBP_ROW(nbp_product_kernel_t2_e2, 2, NBP_EUCLID2, false, false, NBP_PROD_LB(NBP_EUCLID2)),
    NBP_ROW(nbp_product_kernel_t2_e3, 2, NBP_EUCLID3, false, false, NBP_PROD_LB(NBP_EUCLID3)),   NBP_ROW(nbp_product_kernel_t2_ci, 2, NBP_CIRCULAR, false, false, NBP_PROD_LB(NBP_CIRCULAR)),
    NBP_ROW(nbp_product_kernel_t2_se, 2, NBP_SE2, false, false, NBP_PROD_LB(NBP_SE2)),
    NBP_ROW(nbp_product_kernel_t2_e1_xs, 2, NBP_EUCLID1, true, false, NBP_PROD_LB(NBP_EUCLID1)), NBP_ROW(nbp_product_kernel_t2_e2_xs, 2, NBP_EUCLID2, true, false, NBP_PROD_LB(NBP_EUCLID2)),
    NBP_ROW(nbp_product_kernel_t2_e3_xs, 2, NBP_EUCLID3, true, false, NBP_PROD_LB(NBP_EUCLID3)), NBP_ROW(nbp_product_kernel_t2_ci_xs, 2, NBP_CIRCULAR, true, false, NBP_PROD_LB(NBP_CIRCULAR)),
    NBP_ROW(nbp_product_kernel_t2_se_xs, 2, NBP_SE2, true, false, NBP_PROD_LB(NBP_SE2)),
};
#undef NBP_ROW

static int manifold_dim_h(int m) { return m == NBP_SE2 ? 3 : (m == NBP_CIRCULAR ? 1 : m); }
static int manifold_P_h(int m) { return m == NBP_SE2 ? 6 : manifold_dim_h(m); }
static bool manifold_ok(int m) { return m >= NBP_EUCLID1 && m <= NBP_SE2; }
static bool manifold_circ_h(int m, int d) { return (m == NBP_CIRCULAR && d == 0) || (m == NBP_SE2 && d == 2); }  // (is_circ of the device)
static double wrap_h(double a) { return nbpm_wrap_pi(a); }  // (include/nbp_math.h)

// ---- helpers of the batches over resident beliefs (used far below; the templates need C++ linkage, so they stand here) ----------
#define NBPCHK(...)                    \
  do {                                 \
    nbp_status rc_ = (__VA_ARGS__);    \
    if (rc_) return rc_;               \
  } while (0)
struct refusal {
  nbp_status code;
  const char *what;  // nullptr: none
};
static refusal no_refusal(int) { return {NBP_OK, nullptr}; }
// a coordinate bit mask (bit d = coordinate d) names at least one coordinate and none beyond the manifold's
static refusal mask_refusal(int manifold, int32_t mask) {
  if (mask == 0) return {NBP_ERR_RANGE, "empty mask"};
  if (mask < 0 || (mask >> manifold_dim_h(manifold)) != 0) return {NBP_ERR_RANGE, "coordinate outside the manifold"};
  return {NBP_OK, nullptr};
}

template <class K, class... A>
static nbp_status launch_checked(nbp_ctx *c, K kernel, size_t blocks, int lanes, size_t lds, A... args) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(lanes), lds, c->stream, args...);
  HIPCHK(hipGetLastError());
  return NBP_OK;
}

// selects the device; then, element by element and in this order: every slot column, the manifold, what `extra(i)` refuses
// (no_refusal: nothing more)
template <class Extra>
static nbp_status batch_check(nbp_ctx *c, const char *who, std::initializer_list<const int32_t *> slot_cols, const int32_t *manifolds,
                              int n, Extra extra) {
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    refusal r{NBP_OK, nullptr};
    for (const int32_t *s : slot_cols)
      if (s[i] < 0 || s[i] >= c->n_slots) r = {NBP_ERR_RANGE, "slot out of range"};
    if (!r.what && !manifold_ok(manifolds[i])) r = {NBP_ERR_ARG, "unknown manifold"};
    if (!r.what) r = extra(i);
    if (r.what) return fail(r.code, std::string(who) + ": belief " + std::to_string(i) + ": " + r.what);
  }
  return NBP_OK;
}

extern "C" {

int64_t nbp_slot_stride_doubles(int32_t N) { return 3 * (int64_t)N + 8; }
int64_t nbp_arena_bytes(int32_t N, int32_t n_slots) { return nbp_slot_stride_doubles(N) * 8 * (int64_t)n_slots; }
const char *nbp_last_error(void) { return g_err.c_str(); }

// data-independent level tables of the balanced KD-tree over N leaves, on the host: T.N, T.L, T.cnt and T.off, and the arrays
// build_levels uploads
static nbp_status levels_host(int N, nbp_levels &T, std::vector<int32_t> &ints, std::vector<double> &dbls) {
  std::vector<std::vector<int>> lo(1), hi(1), child;
  lo[0] = {0};
  hi[0] = {N};
  int l = 0;
  for (;;) {
    bool all_leaf = true;
    for (size_t k = 0; k < lo[l].size(); k++)
      if (hi[l][k] - lo[l][k] > 1) all_leaf = false;
    if (all_leaf) break;
    lo.emplace_back();
    hi.emplace_back();
    child.emplace_back();
    for (size_t k = 0; k < lo[l].size(); k++) {
      int a = lo[l][k], b = hi[l][k];
      if (b - a == 1) {
        lo[l + 1].push_back(a);
        hi[l + 1].push_back(b);
      } else {
        int mid = a + (b - a + 1) / 2;
        lo[l + 1].push_back(a); hi[l + 1].push_back(mid);
        lo[l + 1].push_back(mid); hi[l + 1].push_back(b);
      }
      child[l].push_back((int)lo[l + 1].size() - 1);
    }
    l++;
    if (l >= NBP_MAXLEVELS - 1) return fail(NBP_ERR_RANGE, "tree too deep");
  }
  const int L = l;
  int total = 0;
  for (int i = 0; i <= L; i++) { T.cnt[i] = (int)lo[i].size(); T.off[i] = total; total += T.cnt[i]; }
  if ((size_t)total > nbp_kd_nodes_cap(N)) return fail(NBP_ERR_RANGE, "level tables exceed the node-sum workspace");
  std::vector<int32_t> nlo(total), nhi(total), nch(total, 0), pos((size_t)(L + 1) * N);
  dbls.resize(2 * (size_t)total);
  for (int i = 0; i <= L; i++)
    for (int k = 0; k < T.cnt[i]; k++) {
      nlo[T.off[i] + k] = lo[i][k];
      nhi[T.off[i] + k] = hi[i][k];
      if (i < L) nch[T.off[i] + k] = child[i][k];
      dbls[T.off[i] + k] = std::log((double)(hi[i][k] - lo[i][k]) / (double)N);
      dbls[total + T.off[i] + k] = (double)(hi[i][k] - lo[i][k]) / (double)N;
      for (int p = lo[i][k]; p < hi[i][k]; p++) pos[(size_t)i * N + p] = k;
    }
  ints.insert(ints.end(), nlo.begin(), nlo.end());
  ints.insert(ints.end(), nhi.begin(), nhi.end());
  ints.insert(ints.end(), nch.begin(), nch.end());
  ints.insert(ints.end(), pos.begin(), pos.end());
  T.N = N;
  T.L = L;
  return NBP_OK;
}
static nbp_status build_levels(nbp_ctx *c) {
  std::vector<int32_t> ints;
  std::vector<double> dbls;
  NBPCHK(levels_host(c->N, c->T, ints, dbls));
  const int total = c->T.off[c->T.L] + c->T.cnt[c->T.L];
  HIPCHK(hipMalloc(&c->lv_ints, ints.size() * 4));
  HIPCHK(hipMalloc(&c->lv_dbls, dbls.size() * 8));
  HIPCHK(hipMemcpy(c->lv_ints, ints.data(), ints.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->lv_dbls, dbls.data(), dbls.size() * 8, hipMemcpyHostToDevice));
  c->T.node_lo = c->lv_ints;
  c->T.node_hi = c->lv_ints + total;
  c->T.node_child = c->lv_ints + 2 * total;
  c->T.pos_node = c->lv_ints + 3 * total;
  c->T.node_logw = c->lv_dbls;
  c->T.node_w = c->lv_dbls + total;
  return NBP_OK;
}

// Everything the launch planners (proposal_plan, fit_plan, product_plan) read of a context besides the level table: the sizes
// that follow from N and the switches of the environment.  nbp_ctx_create and the plan queries (nbp_plan_products, ...) both
// fill a context here, so that a query sees what a context created at that moment would.
static void ctx_plan_fields(nbp_ctx *c, int N) {
  c->N = N;
  c->S = nbp_slot_stride_doubles(N);
  c->Npad = ((N + 63) / 64) * 64;
  c->P = 1024 / c->Npad;
  if (c->P > 4) c->P = 4;
  if (c->P < 1) c->P = 1;
  c->threads = c->P * c->Npad;
  c->spec_on = getenv("NBP_NO_SPECULATIVE_FITS") == nullptr;
  c->spec_depth3 = !(getenv("NBP_SPEC_DEPTH3") && atoi(getenv("NBP_SPEC_DEPTH3")) == 0);
  c->fused_on = getenv("NBP_NO_FUSED_UPDATE") == nullptr;
  if (getenv("NBP_FUSED_MIN")) c->fused_min = atoi(getenv("NBP_FUSED_MIN"));
  if (getenv("NBP_PROPOSAL_WAVE_MIN")) c->prop_wave_min = atoi(getenv("NBP_PROPOSAL_WAVE_MIN"));
  if (getenv("NBP_PROPOSAL_SPLIT_MIN")) c->prop_split_min = atoi(getenv("NBP_PROPOSAL_SPLIT_MIN"));
  if (getenv("NBP_PIPELINE_MIN")) c->pipe_min = atoi(getenv("NBP_PIPELINE_MIN"));
  c->no_lanes = getenv("NBP_NO_LANES") && atoi(getenv("NBP_NO_LANES")) != 0;
  c->no_sinks = getenv("NBP_NO_SINKS") && atoi(getenv("NBP_NO_SINKS")) != 0;
  if (getenv("NBP_SINK_PLACEMENT")) c->sink_placement = atoi(getenv("NBP_SINK_PLACEMENT"));
  if (getenv("NBP_FUSED_P1_MIN")) c->fused_p1_min = atoi(getenv("NBP_FUSED_P1_MIN"));
  if (getenv("NBP_PRODUCT_HL2_MIN")) c->prod_hl2_min = atoi(getenv("NBP_PRODUCT_HL2_MIN"));
  if (getenv("NBP_PRODUCT_NCH")) c->prod_nch = atoi(getenv("NBP_PRODUCT_NCH"));
  if (getenv("NBP_PRODUCT_ALL_LEVELS_HL")) c->prod_all_levels_hl = atoi(getenv("NBP_PRODUCT_ALL_LEVELS_HL"));
  c->prod_xs = getenv("NBP_NO_XS_PRODUCTS") == nullptr;
  c->prod_lat_uni = getenv("NBP_NO_UNIFORM_LATENCY_PRODUCTS") == nullptr;
  if (getenv("NBP_LCV_P2_MIN")) c->lcv_p2_min = atoi(getenv("NBP_LCV_P2_MIN"));
  if (getenv("NBP_LCV_P1_MIN")) c->lcv_p1_min = atoi(getenv("NBP_LCV_P1_MIN"));
  c->fit_w5 = getenv("NBP_NO_W5_FITS") == nullptr;
  c->debug_occupancy = getenv("NBP_DEBUG_OCCUPANCY") != nullptr;
}

nbp_status nbp_ctx_create(int32_t device, int32_t N, int32_t n_slots, void *arena, int64_t arena_bytes,
                          int32_t side_ints, nbp_ctx **out) {
  if (!out) return fail(NBP_ERR_ARG, "out is null");
  if (N < 8 || N > NBP_MAXN) return fail(NBP_ERR_RANGE, "N must be in [8, 512]");
  if (n_slots < 1) return fail(NBP_ERR_ARG, "n_slots < 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(NBP_ERR_NOGPU, "no HIP device visible: libnbp has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(NBP_ERR_ARG, "bad device index");
  HIPCHK(hipSetDevice(device));
  nbp_ctx *c = new nbp_ctx();
  // any failure below releases the half-built context (stream, side buffer, counters, arena)
  struct guard_t {
    nbp_ctx *c;
    ~guard_t() { if (c) nbp_ctx_destroy(c); }
  } guard{c};
  c->device = device;
  c->n_slots = n_slots;
  ctx_plan_fields(c, N);
  c->side_ints = side_ints > 0 ? side_ints : 1;
  if (arena) {
    if (arena_bytes < nbp_arena_bytes(N, n_slots)) return fail(NBP_ERR_ARG, "arena too small");
    c->arena = (double *)arena;
  } else {
    HIPCHK(hipMalloc(&c->arena, nbp_arena_bytes(N, n_slots)));
    HIPCHK(hipMemset(c->arena, 0, nbp_arena_bytes(N, n_slots)));
    c->own_arena = true;
  }
  HIPCHK(hipMalloc(&c->side, (size_t)c->side_ints * 4));
  HIPCHK(hipMemset(c->side, 0, (size_t)c->side_ints * 4));
  HIPCHK(hipMalloc(&c->counters, sizeof(nbp_counters)));
  HIPCHK(hipMemset(c->counters, 0, sizeof(nbp_counters)));
  {  // NBP_FIT_F64=1: the bandwidth searches evaluate in double precision only (no single-precision bracketing, neg_loo_ll_f32)
    const char *e = getenv("NBP_FIT_F64");
    const unsigned long long fl = (e && *e && *e != '0') ? 1ull : 0ull;
    HIPCHK(hipMemcpy(&c->counters->flags, &fl, sizeof(fl), hipMemcpyHostToDevice));
  }
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipMalloc(&c->spec, sizeof(nbp_spec_area) * 3 * NBP_SPEC_MAXJOBS * 2));  // (the second half: lane 1 of a program)
  HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) HIPCHK(hipEventCreateWithFlags(&c->pipe_ev[i], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->lane_join, hipEventDisableTiming));
  nbp_status rc = build_levels(c);
  if (rc != NBP_OK) return rc;
  // allow the full 160 KiB LDS for the product kernels
  for (const nbp_product_kernel_row &k : NBP_PRODUCT_KERNELS)
    HIPCHK(hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  for (const void *k : {(const void *)nbp_bandwidth_kernel, (const void *)nbp_prep_kernel, (const void *)nbp_bandwidth_kernel_spec<2>,
                        (const void *)nbp_bandwidth_kernel_spec<3>, (const void *)nbp_prep_kernel_spec<2>, (const void *)nbp_prep_kernel_spec<3>})
    HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  // (the kernel has 608 B of static LDS, the hypothesis recipe: static + dynamic must stay within the 160 KiB)
  HIPCHK(hipFuncSetAttribute((const void *)nbp_update_kernel_lin2_p1, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)nbp_update_kernel_lin2_p2, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));

  guard.c = nullptr;
  *out = c;
  return NBP_OK;
}

static void program_detach(nbp_program *p);
static void program_delete(nbp_program *p);  // detach + delete (defined behind the type)
static void ctx_detach_comms(nbp_ctx *c);
static void heatmap_release(nbp_heatmap *hm);  // frees the device memory, leaves the context
static void reap_retired(nbp_ctx *c);

nbp_status nbp_ctx_attach(nbp_ctx *c, void *obj, void (*destroy)(void *)) {
  if (!c) return fail(NBP_ERR_ARG, "ctx is null");
  if (c->attached && c->attached_destroy && c->attached != obj) c->attached_destroy(c->attached);
  c->attached = obj;
  c->attached_destroy = destroy;
  return NBP_OK;
}
void *nbp_ctx_attached(const nbp_ctx *c) { return c ? c->attached : nullptr; }

nbp_status nbp_ctx_destroy(nbp_ctx *c) {
  if (!c) return NBP_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->attached && c->attached_destroy) c->attached_destroy(c->attached);  // (may destroy programs of this context: first)
  c->attached = nullptr;
  for (nbp_program *p : c->programs) program_detach(p);  // a program outliving its context must not touch it
  c->programs.clear();
  while (!c->heatmaps.empty()) heatmap_release(c->heatmaps.back());  // likewise a heatmap density: its handle stays valid for nbp_heatmap_destroy
  ctx_detach_comms(c);  // likewise a communicator: shut down now, its handle stays valid for nbp_comm_destroy
  for (auto &v : c->ev)
    for (auto &p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
  if (c->own_arena) hipFree(c->arena);
  if (c->side) hipFree(c->side);
  if (c->counters) hipFree(c->counters);
  if (c->lv_ints) hipFree(c->lv_ints);
  if (c->lv_dbls) hipFree(c->lv_dbls);
  if (c->stage) hipFree(c->stage);
  if (c->query) hipFree(c->query);
  if (c->pin) hipHostFree(c->pin);
  for (auto &b : c->blob_cache) hipFree(b.first);
  c->blob_cache.clear();
  // the programs handed to nbp_program_retire that are still pending: the caller gave up ownership there, so they end here
  // (the stream was synchronised above: everything they queued has run; detached like the live ones, then deleted)
  for (auto &r : c->retired) {
    hipEventDestroy(r.second);
    program_delete(r.first);
  }
  c->retired.clear();
  for (nbp_ctx::pin_buf *b : c->pin_pool) {
    if (b->p) hipHostFree(b->p);
    if (b->ev) hipEventDestroy(b->ev);
    delete b;
  }
  c->pin_pool.clear();
  if (c->ws) hipFree(c->ws);
  if (c->gstats) hipFree(c->gstats);
  if (c->spec) hipFree(c->spec);
  if (c->stream2) hipStreamDestroy(c->stream2);
  for (int i = 0; i < 2; i++) if (c->pipe_ev[i]) hipEventDestroy(c->pipe_ev[i]);
  for (hipEvent_t e : c->lane_ev) hipEventDestroy(e);
  if (c->lane_fork) hipEventDestroy(c->lane_fork);
  if (c->lane_join) hipEventDestroy(c->lane_join);
  if (c->gstats1) hipFree(c->gstats1);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return NBP_OK;
}

nbp_status nbp_synchronize(nbp_ctx *c) {
  if (!c) return fail(NBP_ERR_ARG, "ctx is null");
  HIPCHK(hipStreamSynchronize(c->stream));
  reap_retired(c);
  return NBP_OK;
}
void *nbp_arena_ptr(nbp_ctx *c) { return c ? c->arena : nullptr; }
void *nbp_stream_ptr(nbp_ctx *c) { return c ? (void *)c->stream : nullptr; }
int32_t nbp_ctx_particles(const nbp_ctx *c) { return c ? c->N : 0; }
int32_t nbp_ctx_slots(const nbp_ctx *c) { return c ? c->n_slots : 0; }
int32_t nbp_ctx_device(const nbp_ctx *c) { return c ? c->device : -1; }
int32_t nbp_ctx_resident(const nbp_ctx *c) { return c ? c->resident : 0; }
nbp_status nbp_ctx_reserve_resident(nbp_ctx *c, int32_t n) {
  if (!c) return fail(NBP_ERR_ARG, "ctx is null");
  if (n < 0 || n > c->n_slots) return fail(NBP_ERR_RANGE, "resident slots: more than the context holds");
  c->resident = n;
  return NBP_OK;
}

// a pinned buffer nobody holds and no queued copy still reads (or a new one)
static nbp_ctx::pin_buf *pin_acquire(nbp_ctx *c, size_t bytes) {
  nbp_ctx::pin_buf *best = nullptr;
  for (nbp_ctx::pin_buf *b : c->pin_pool) {
    if (b->held) continue;
    if (b->pending) {
      if (hipEventQuery(b->ev) != hipSuccess) continue;
      b->pending = false;
    }
    if (b->bytes >= bytes && (!best || b->bytes < best->bytes)) best = b;
  }
  if (!best) {
    best = new nbp_ctx::pin_buf();
    const size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 2;
    if (hipHostMalloc((void **)&best->p, cap, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&best->ev, hipEventDisableTiming) != hipSuccess) {
      if (best->p) hipHostFree(best->p);
      delete best;
      return nullptr;
    }
    best->bytes = cap;
    c->pin_pool.push_back(best);
  }
  best->held = true;
  return best;
}
// free once everything queued on the library stream so far has run (the copies out of / into the buffer among it)
static void pin_release_behind_stream(nbp_ctx *c, nbp_ctx::pin_buf *b) {
  b->pending = hipEventRecord(b->ev, c->stream) == hipSuccess;
  b->held = false;
}

// ---- belief I/O --------------------------------------------------------------------------------
nbp_status nbp_slot_write(nbp_ctx *c, int32_t slot, int32_t manifold, const double *pts, const double *bw) {
  return nbp_belief_write(c, slot, manifold, pts, c ? c->N : 0, bw, nullptr);
}
nbp_status nbp_slot_read(nbp_ctx *c, int32_t slot, int32_t manifold, double *pts, double *bw) {
  return nbp_belief_read(c, slot, manifold, pts, nullptr, bw, nullptr);
}

// a belief as its slot holds it: coordinates SoA over N rows, then bandwidth (3), infoPerCoord (3), count
static void pack_belief(const nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, const double *ipc, double *s) {
  const int N = c->N, D = manifold_dim_h(manifold), P = manifold_P_h(manifold);
  memset(s, 0, sizeof(double) * (size_t)c->S);
  const int cnt = n_pts < N ? n_pts : N;  // more than N points: the first N (GraphProductOperations.jl:44, `_pts[1:N]`)
  s[3 * N + 6] = cnt < N ? (double)cnt : 0.0;
  for (int n = 0; n < cnt; n++) {
    const double *p = pts + (size_t)n * P;
    if (manifold == NBP_SE2) {
      s[n] = p[0];
      s[N + n] = p[1];
      s[2 * N + n] = nbpm_atan2(p[3], p[2]);  // (the shared atan2, include/nbp_math.h: the CPU checker converts with the same function)
    } else if (manifold == NBP_CIRCULAR) {
      s[n] = wrap_h(p[0]);
    } else {
      for (int d = 0; d < D; d++) s[d * N + n] = p[d];
    }
  }
  for (int d = 0; d < D; d++) s[3 * N + d] = bw ? bw[d] : 0.0;
  for (int d = 0; d < D; d++) s[3 * N + 3 + d] = ipc ? ipc[d] : 0.0;  // a fresh VariableNodeData carries infoPerCoord = 0
}
// with n_pts: the rows the belief holds (the caller sized `pts` by the count it expects back, at most N); without
// (nbp_slot_read): all N rows of the slot
static void unpack_belief(const nbp_ctx *c, int32_t manifold, const double *s, double *pts, int32_t *n_pts, double *bw, double *ipc) {
  const int N = c->N, D = manifold_dim_h(manifold), P = manifold_P_h(manifold);
  const int cnt_held = (s[3 * N + 6] > 0.0 && s[3 * N + 6] < (double)N) ? (int)s[3 * N + 6] : N;
  const int rows = n_pts ? cnt_held : N;
  for (int n = 0; n < rows; n++) {
    double *p = pts + (size_t)n * P;
    if (manifold == NBP_SE2) {
      double th = s[2 * N + n];
      p[0] = s[n]; p[1] = s[N + n];
      double sn, cs;
      nbpm_sincos(th, &sn, &cs);  // (the shared sincos: a libm's cos / sin and its fused sincos round differently now and then)
      p[2] = cs; p[3] = sn; p[4] = -sn; p[5] = cs;
    } else {
      for (int d = 0; d < D; d++) p[d] = s[d * N + n];
    }
  }
  if (bw)
    for (int d = 0; d < D; d++) bw[d] = s[3 * N + d];
  if (ipc)
    for (int d = 0; d < D; d++) ipc[d] = s[3 * N + 3 + d];
  if (n_pts) *n_pts = cnt_held;
}
static nbp_status belief_args(nbp_ctx *c, int32_t slot, int32_t manifold, const double *pts) {
  if (!c || !pts) return fail(NBP_ERR_ARG, "null argument");
  if (slot < 0 || slot >= c->n_slots) return fail(NBP_ERR_RANGE, "slot out of range");
  if (!manifold_ok(manifold)) return fail(NBP_ERR_ARG, "unknown manifold");
  return NBP_OK;
}

nbp_status nbp_belief_write(nbp_ctx *c, int32_t slot, int32_t manifold, const double *pts, int32_t n_pts, const double *bw,
                            const double *ipc) {
  nbp_status rc = belief_args(c, slot, manifold, pts);
  if (rc) return rc;
  if (n_pts < 1) return fail(NBP_ERR_RANGE, "belief: n_pts < 1");
  if (n_pts < c->N && !bw) return fail(NBP_ERR_ARG, "belief: a belief with fewer than N points needs its bandwidth (it is a density, not a point set)");
  std::vector<double> s(c->S);
  pack_belief(c, manifold, pts, n_pts, bw, ipc, s.data());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->arena + c->S * slot, s.data(), c->S * 8, hipMemcpyHostToDevice));
  return NBP_OK;
}

nbp_status nbp_belief_read(nbp_ctx *c, int32_t slot, int32_t manifold, double *pts, int32_t *n_pts, double *bw, double *ipc) {
  nbp_status rc = belief_args(c, slot, manifold, pts);
  if (rc) return rc;
  std::vector<double> s(c->S);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(s.data(), c->arena + c->S * slot, c->S * 8, hipMemcpyDeviceToHost));
  unpack_belief(c, manifold, s.data(), pts, n_pts, bw, ipc);
  return NBP_OK;
}

// ---- many beliefs in one call ---------------------------------------------------------------------------------------------
// The beliefs are packed into (unpacked from) a pinned staging buffer and moved with ONE asynchronous copy per run of
// consecutive slots on the library stream: a clique call moves its 3-10 beliefs in one or two copies instead of one
// synchronous copy each, a caller that loads a whole graph moves it in one.
static nbp_status ensure_pin(nbp_ctx *c, size_t doubles) {
  if (doubles <= c->pin_doubles) return NBP_OK;
  if (c->pin) HIPCHK(hipHostFree(c->pin));
  c->pin = nullptr;
  c->pin_doubles = 0;
  const size_t cap = doubles * 2;
  static const bool noncoh = getenv("NBP_PIN_NONCOHERENT") != nullptr;
  HIPCHK(hipHostMalloc((void **)&c->pin, cap * 8, noncoh ? hipHostMallocNonCoherent : hipHostMallocDefault));
  c->pin_doubles = cap;
  return NBP_OK;
}
// The beliefs of a batch are staged IN SLOT ORDER, so that every run of consecutive slots is one copy whatever order the caller
// names them in: resident handles count down from the end of the arena (handle h = slot n_slots - h), and a graph of a thousand
// beliefs written or read through its handles was a thousand copies of 4.9 KB (round 6: 1813 `copyBuffer` launches per queued walk
// of the clique seam, ~3 ms of device time and twice that in launch gaps; tools/exp/seam_walk_trace.sh).  ord[k] = the request
// staged at position k (stable: a slot named twice keeps the caller's order).
static std::vector<int> slot_order(int n, const int32_t *slots) {
  std::vector<int> ord((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) ord[(size_t)i] = i;
  bool asc = true;
  for (int i = 1; i < n && asc; i++) asc = slots[i] >= slots[i - 1];
  if (!asc) std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return slots[a] < slots[b]; });
  return ord;
}

nbp_status nbp_belief_write_batch(nbp_ctx *c, int32_t n, const int32_t *slots, const int32_t *manifolds, const double *const *pts,
                                  const int32_t *n_pts, const double *const *bw, const double *const *ipc) {
  if (!c || (n > 0 && (!slots || !manifolds || !pts))) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    nbp_status rc = belief_args(c, slots[i], manifolds[i], pts[i]);
    if (rc) return rc;
    const int np = n_pts ? n_pts[i] : c->N;
    if (np < 1) return fail(NBP_ERR_RANGE, "belief: n_pts < 1");
    if (np < c->N && !(bw && bw[i])) return fail(NBP_ERR_ARG, "belief: a belief with fewer than N points needs its bandwidth (it is a density, not a point set)");
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // the staging buffer is free again (and so is every slot about to be replaced)
  nbp_status rc = ensure_pin(c, (size_t)n * (size_t)c->S);
  if (rc) return rc;
  const std::vector<int> ord = slot_order(n, slots);
  host_parallel_for(n, 128, [&](int k) {
    const int i = ord[(size_t)k];
    pack_belief(c, manifolds[i], pts[i], n_pts ? n_pts[i] : c->N, bw ? bw[i] : nullptr, ipc ? ipc[i] : nullptr, c->pin + (size_t)k * c->S);
  });
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && slots[ord[(size_t)j]] == slots[ord[(size_t)j - 1]] + 1) j++;
    HIPCHK(hipMemcpyAsync(c->arena + c->S * slots[ord[(size_t)i]], c->pin + (size_t)i * c->S, (size_t)(j - i) * c->S * 8, hipMemcpyHostToDevice, c->stream));
    i = j;
  }
  return NBP_OK;  // stream-ordered: whatever is launched next sees the beliefs; the next use of the staging buffer waits for the copies
}
nbp_status nbp_belief_read_batch(nbp_ctx *c, int32_t n, const int32_t *slots, const int32_t *manifolds, double *const *pts,
                                 int32_t *n_pts, double *const *bw, double *const *ipc) {
  if (!c || (n > 0 && (!slots || !manifolds || !pts))) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    nbp_status rc = belief_args(c, slots[i], manifolds[i], pts[i]);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  // ascending slots with small gaps (the updated variables of many cliques): reading the gaps along costs less than a copy
  // per run -- one copy of the whole span while it stays under four times the bytes asked for
  const std::vector<int> ord = slot_order(n, slots);  // (in slot order: see slot_order)
  const int32_t s_lo = slots[ord[0]], s_hi = slots[ord[(size_t)n - 1]];
  bool strictly = true;
  for (int k = 1; k < n; k++) strictly &= slots[ord[(size_t)k]] > slots[ord[(size_t)k - 1]];
  const size_t span = strictly ? (size_t)(s_hi - s_lo + 1) : 0;
  if (strictly && span > (size_t)n && span <= 4 * (size_t)n) {
    nbp_status rc = ensure_pin(c, span * (size_t)c->S);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->pin, c->arena + c->S * s_lo, span * c->S * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    host_parallel_for(n, 128, [&](int i) {
      unpack_belief(c, manifolds[i], c->pin + (size_t)(slots[i] - s_lo) * c->S, pts[i], n_pts ? &n_pts[i] : nullptr, bw ? bw[i] : nullptr,
                    ipc ? ipc[i] : nullptr);
    });
    return NBP_OK;
  }
  nbp_status rc = ensure_pin(c, (size_t)n * (size_t)c->S);
  if (rc) return rc;
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && slots[ord[(size_t)j]] == slots[ord[(size_t)j - 1]] + 1) j++;
    HIPCHK(hipMemcpyAsync(c->pin + (size_t)i * c->S, c->arena + c->S * slots[ord[(size_t)i]], (size_t)(j - i) * c->S * 8, hipMemcpyDeviceToHost, c->stream));
    i = j;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  host_parallel_for(n, 128, [&](int k) {
    const int i = ord[(size_t)k];
    unpack_belief(c, manifolds[i], c->pin + (size_t)k * c->S, pts[i], n_pts ? &n_pts[i] : nullptr, bw ? bw[i] : nullptr, ipc ? ipc[i] : nullptr);
  });
  return NBP_OK;
}

// The same transfers WITHOUT a host synchronisation (the asynchronous clique seam): staged in a buffer of the context's pool.
nbp_status nbp_belief_write_batch_async(nbp_ctx *c, int32_t n, const int32_t *slots, const int32_t *manifolds, const double *const *pts,
                                        const int32_t *n_pts, const double *const *bw, const double *const *ipc) {
  if (!c || (n > 0 && (!slots || !manifolds || !pts))) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    nbp_status rc = belief_args(c, slots[i], manifolds[i], pts[i]);
    if (rc) return rc;
    const int np = n_pts ? n_pts[i] : c->N;
    if (np < 1) return fail(NBP_ERR_RANGE, "belief: n_pts < 1");
    if (np < c->N && !(bw && bw[i])) return fail(NBP_ERR_ARG, "belief: a belief with fewer than N points needs its bandwidth (it is a density, not a point set)");
  }
  nbp_ctx::pin_buf *b = pin_acquire(c, (size_t)n * (size_t)c->S * 8);
  if (!b) return fail(NBP_ERR_HIP, "pinned staging buffer");
  double *pin = (double *)b->p;
  const std::vector<int> ord = slot_order(n, slots);
  host_parallel_for(n, 128, [&](int k) {
    const int i = ord[(size_t)k];
    pack_belief(c, manifolds[i], pts[i], n_pts ? n_pts[i] : c->N, bw ? bw[i] : nullptr, ipc ? ipc[i] : nullptr, pin + (size_t)k * c->S);
  });
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && slots[ord[(size_t)j]] == slots[ord[(size_t)j - 1]] + 1) j++;
    if (hipMemcpyAsync(c->arena + c->S * slots[ord[(size_t)i]], pin + (size_t)i * c->S, (size_t)(j - i) * c->S * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
      pin_release_behind_stream(c, b);
      return fail(NBP_ERR_HIP, "hipMemcpyAsync (beliefs in)");
    }
    i = j;
  }
  pin_release_behind_stream(c, b);
  return NBP_OK;
}
struct nbp_read_token {
  nbp_ctx *ctx;
  nbp_ctx::pin_buf *buf;
  hipEvent_t done;
  std::vector<int32_t> slots;
  std::vector<int> ord;  // staging position -> request (slot order: slot_order)
};
nbp_status nbp_belief_read_batch_begin(nbp_ctx *c, int32_t n, const int32_t *slots, nbp_read_token **out) {
  if (!c || !out || (n > 0 && !slots)) return fail(NBP_ERR_ARG, "null argument");
  *out = nullptr;
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= c->n_slots) return fail(NBP_ERR_RANGE, "slot out of range");
  nbp_read_token *t = new nbp_read_token();
  t->ctx = c;
  t->buf = nullptr;
  t->done = nullptr;
  t->slots.assign(slots, slots + (n > 0 ? n : 0));
  if (hipEventCreateWithFlags(&t->done, hipEventDisableTiming) != hipSuccess) { delete t; return fail(NBP_ERR_HIP, "hipEventCreate"); }
  if (n > 0) {
    t->buf = pin_acquire(c, (size_t)n * (size_t)c->S * 8);
    if (!t->buf) { hipEventDestroy(t->done); delete t; return fail(NBP_ERR_HIP, "pinned staging buffer"); }
    double *pin = (double *)t->buf->p;
    t->ord = slot_order(n, slots);
    const std::vector<int> &ord = t->ord;
    for (int i = 0; i < n;) {
      int j = i + 1;
      while (j < n && slots[ord[(size_t)j]] == slots[ord[(size_t)j - 1]] + 1) j++;
      if (hipMemcpyAsync(pin + (size_t)i * c->S, c->arena + c->S * slots[ord[(size_t)i]], (size_t)(j - i) * c->S * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        pin_release_behind_stream(c, t->buf);
        hipEventDestroy(t->done);
        delete t;
        return fail(NBP_ERR_HIP, "hipMemcpyAsync (beliefs out)");
      }
      i = j;
    }
  }
  if (hipEventRecord(t->done, c->stream) != hipSuccess) {
    if (t->buf) pin_release_behind_stream(c, t->buf);
    hipEventDestroy(t->done);
    delete t;
    return fail(NBP_ERR_HIP, "hipEventRecord");
  }
  *out = t;
  return NBP_OK;
}
// waits for the copies of `begin` (and everything queued before them), unpacks; the token is gone afterwards, whatever the status
nbp_status nbp_belief_read_batch_end(nbp_read_token *t, const int32_t *manifolds, double *const *pts, int32_t *n_pts, double *const *bw,
                                     double *const *ipc) {
  if (!t) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx *c = t->ctx;
  const int n = (int)t->slots.size();
  const hipError_t e = hipEventSynchronize(t->done);
  nbp_status rc = NBP_OK;
  if (e != hipSuccess) rc = fail(NBP_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
  else if (n > 0 && (!manifolds || !pts)) rc = fail(NBP_ERR_ARG, "null argument");
  else if (n > 0) {
    const double *pin = (const double *)t->buf->p;
    host_parallel_for(n, 128, [&](int k) {
      const int i = t->ord[(size_t)k];
      if (pts[i]) unpack_belief(c, manifolds[i], pin + (size_t)k * c->S, pts[i], n_pts ? &n_pts[i] : nullptr, bw ? bw[i] : nullptr, ipc ? ipc[i] : nullptr);
    });
  }
  if (t->buf) { t->buf->held = false; t->buf->pending = false; }
  hipEventDestroy(t->done);
  delete t;
  return rc;
}

nbp_status nbp_side_write(nbp_ctx *c, int32_t offset, const int32_t *src, int32_t n) {
  if (!c || !src) return fail(NBP_ERR_ARG, "null argument");
  if (offset < 0 || n < 0 || offset + n > c->side_ints) return fail(NBP_ERR_RANGE, "side buffer range");
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->side + offset, src, (size_t)n * 4, hipMemcpyHostToDevice));
  return NBP_OK;
}
nbp_status nbp_side_read(nbp_ctx *c, int32_t offset, int32_t *dst, int32_t n) {
  if (!c || !dst) return fail(NBP_ERR_ARG, "null argument");
  if (offset < 0 || n < 0 || offset + n > c->side_ints) return fail(NBP_ERR_RANGE, "side buffer range");
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(dst, c->side + offset, (size_t)n * 4, hipMemcpyDeviceToHost));
  return NBP_OK;
}

// ---- validation ----------------------------------------------------------------------------------
static nbp_status check_proposals(nbp_ctx *c, const nbp_proposal_desc *d, int n) {
  for (int i = 0; i < n; i++) {
    const nbp_proposal_desc &p = d[i];
    if (!manifold_ok(p.manifold)) return fail(NBP_ERR_ARG, "proposal: unknown manifold");
    if (p.factor_kind < NBP_F_PRIOR || p.factor_kind > NBP_F_PASSTHROUGH) return fail(NBP_ERR_ARG, "proposal: unknown factor kind");
    if (p.factor_kind == NBP_F_PASSTHROUGH) {  // the density is the proposal: a unary factor, two slots, an optional partial mask
      if (p.nvars != 1 || p.sfidx != 0) return fail(NBP_ERR_ARG, "proposal: a pass-through prior is unary");
      if (p.out_slot < 0 || p.out_slot >= c->n_slots) return fail(NBP_ERR_RANGE, "proposal: out_slot");
      for (int k = 0; k < 2; k++)
        if (p.var_slot[k] < 0 || p.var_slot[k] >= c->n_slots) return fail(NBP_ERR_RANGE, "proposal: var_slot");
      if (p.partial_mask < 0 || p.partial_mask >= (1 << manifold_dim_h(p.manifold))) return fail(NBP_ERR_RANGE, "proposal: partial_mask");
      if (p.has_multihypo || p.nullhypo != 0.0) return fail(NBP_ERR_ARG, "proposal: a pass-through prior takes no multihypo / nullhypo (evalFactor is bypassed)");
      if (p.keep_count < 0 || p.keep_count > 2) return fail(NBP_ERR_RANGE, "proposal: keep_count");
      continue;
    }
    if (p.nvars < 1 || p.nvars > NBP_MAXV) return fail(NBP_ERR_RANGE, "proposal: nvars");
    if (p.sfidx < 0 || p.sfidx >= p.nvars) return fail(NBP_ERR_RANGE, "proposal: sfidx");
    if (p.ncomp < 1 || p.ncomp > NBP_MAXC) return fail(NBP_ERR_RANGE, "proposal: ncomp");
    if (p.inflate_cycles < 0 || p.inflate_cycles > 8) return fail(NBP_ERR_RANGE, "proposal: inflate_cycles");
    if (p.out_slot < 0 || p.out_slot >= c->n_slots) return fail(NBP_ERR_RANGE, "proposal: out_slot");
    int nv = (p.factor_kind == NBP_F_MSGPRIOR) ? 2 : p.nvars;
    for (int k = 0; k < nv; k++)
      if (p.var_slot[k] < 0 || p.var_slot[k] >= c->n_slots) return fail(NBP_ERR_RANGE, "proposal: var_slot");
    if ((p.factor_kind == NBP_F_PRIOR || p.factor_kind == NBP_F_MSGPRIOR) && p.nvars != 1)
      return fail(NBP_ERR_ARG, "proposal: priors are unary");
    if (p.factor_kind >= NBP_F_LINREL && p.nvars < 2) return fail(NBP_ERR_ARG, "proposal: relative factor needs >= 2 variables");
    if (p.factor_kind >= NBP_F_LINREL && !p.has_multihypo && p.nvars != 2)
      return fail(NBP_ERR_ARG, "proposal: binary mechanics without multihypo needs nvars == 2");
    if (p.factor_kind == NBP_F_CIRCULAR && p.manifold != NBP_CIRCULAR) return fail(NBP_ERR_ARG, "CircularCircular needs Circular variables");
    if (p.factor_kind == NBP_F_SE2 && p.manifold != NBP_SE2) return fail(NBP_ERR_ARG, "SE2 factor needs SE2 variables");
    if (p.factor_kind == NBP_F_LINREL && p.manifold > NBP_EUCLID3) return fail(NBP_ERR_ARG, "LinearRelative needs Euclid variables");
    if (p.mhidx_in >= 0 && p.mhidx_in + c->N > c->side_ints) return fail(NBP_ERR_RANGE, "proposal: mhidx_in");
    if (p.mhidx_out >= 0 && p.mhidx_out + c->N > c->side_ints) return fail(NBP_ERR_RANGE, "proposal: mhidx_out");
    if (p.partial_mask) {
      const int D = manifold_dim_h(p.manifold);
      if (p.partial_mask < 0 || p.partial_mask >= (1 << D)) return fail(NBP_ERR_RANGE, "proposal: partial_mask");
      if (p.factor_kind == NBP_F_LINREL) {
        if (__builtin_popcount(p.partial_mask) > 2) return fail(NBP_ERR_ARG, "partial LinearRelative: one or two partial coordinates");
      } else if (p.factor_kind != NBP_F_PRIOR && p.factor_kind != NBP_F_SE2)
        return fail(NBP_ERR_ARG, "proposal: partial_mask is supported for Prior, LinearRelative and SE(2) ManifoldFactor factors");
    }
    if (p.meas_kde) {
      if (p.meas_kde < 0 || p.meas_kde > c->n_slots) return fail(NBP_ERR_RANGE, "proposal: meas_kde");
      if (p.factor_kind != NBP_F_LINREL && p.factor_kind != NBP_F_CIRCULAR && p.factor_kind != NBP_F_SE2)
        return fail(NBP_ERR_ARG, "proposal: a KDE measurement needs a relative factor whose measurement lives on the variable's manifold");
      if (p.partial_mask) return fail(NBP_ERR_ARG, "proposal: a KDE measurement cannot be partial");
    }
    if (p.has_multihypo) {
      int ncert = 0;
      for (int k = 0; k < p.nvars; k++) ncert += (p.multihypo[k] == 0.0);
      if (ncert != 1) return fail(NBP_ERR_ARG, "proposal: multihypo needs exactly one certain variable (binary mechanics)");
    }
  }
  return NBP_OK;
}
static nbp_status check_products(nbp_ctx *c, const nbp_product_desc *d, int n) {
  for (int i = 0; i < n; i++) {
    const nbp_product_desc &p = d[i];
    if (!manifold_ok(p.manifold)) return fail(NBP_ERR_ARG, "product: unknown manifold");
    if (p.nfactors < 1 || p.nfactors > NBP_MAXF) return fail(NBP_ERR_RANGE, "product: nfactors");
    if (p.niter < 1 || p.niter > 8) return fail(NBP_ERR_RANGE, "product: niter (1 .. 8)");
    if (p.out_slot < 0 || p.out_slot >= c->n_slots) return fail(NBP_ERR_RANGE, "product: out_slot");
    for (int k = 0; k < p.nfactors; k++)
      if (p.in_slot[k] < 0 || p.in_slot[k] >= c->n_slots) return fail(NBP_ERR_RANGE, "product: in_slot");
    if (p.labels_out >= 0 && p.labels_out + c->N * p.nfactors > c->side_ints) return fail(NBP_ERR_RANGE, "product: labels_out");
    {
      const int D = manifold_dim_h(p.manifold);
      bool any = false;
      for (int k = 0; k < p.nfactors; k++) {
        if (p.in_partial[k] >= (1 << D)) return fail(NBP_ERR_RANGE, "product: in_partial");
        any |= (p.in_partial[k] != 0);
      }
      if (any && D < 2) return fail(NBP_ERR_ARG, "product: partial densities need a variable of dimension >= 2");
      if (any && (p.old_slot < 0 || p.old_slot >= c->n_slots)) return fail(NBP_ERR_RANGE, "product: old_slot");
    }
  }
  return NBP_OK;
}
static nbp_status check_copies(nbp_ctx *c, const nbp_copy_desc *d, int n) {
  for (int i = 0; i < n; i++)
    if (d[i].src_slot < 0 || d[i].src_slot >= c->n_slots || d[i].dst_slot < 0 || d[i].dst_slot >= c->n_slots)
      return fail(NBP_ERR_RANGE, "copy: slot out of range");
  return NBP_OK;
}

// ---- launches --------------------------------------------------------------------------------------
static nbp_status tic(nbp_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> &v) {
  if (!c->timing) return NBP_OK;
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  HIPCHK(hipEventRecord(a, c->stream));
  v.emplace_back(a, b);
  return NBP_OK;
}
static nbp_status toc(nbp_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> &v) {
  if (!c->timing) return NBP_OK;
  HIPCHK(hipEventRecord(v.back().second, c->stream));
  return NBP_OK;
}

// What a launch runs with: the stream, the KD workspace it may use and, inside a two-stream round, the size of the WHOLE
// batch (products, and workgroups of its prep launch), by which both halves pick their geometry so that no result depends
// on the split.  geom_n = geom_blocks = 0 outside a round.  By value: nothing a launch does depends on context state that
// a round would have to set and put back.
struct nbp_launch_env {
  hipStream_t stream = nullptr;
  double *ws = nullptr;
  size_t ws_doubles = 0;
  int geom_n = 0, geom_blocks = 0;
  // a lane of a program (run_lanes): 0 = none; 1, 2 = lane 0, lane 1.  Its share of the workspace is fixed (sized at
  // nbp_program_finalize: the other lane's launches are in flight beside it); lane 1 has the second rendezvous area and the
  // second statistics area
  int lane = 0;
};
static nbp_launch_env ctx_env(const nbp_ctx *c) { return {c->stream, c->ws, c->ws_doubles, 0, 0, 0}; }
static nbp_spec_area *env_spec(const nbp_ctx *c, const nbp_launch_env &env) { return c->spec + (env.lane == 2 ? 3 * NBP_SPEC_MAXJOBS : 0); }

// 0, or the class of a batch whose relative factors are all full (non-partial) factors of one kind on one manifold, with
// everything else in it (priors, message priors, pass-through densities) on that manifold as well: LinearRelative on
// Euclid(2) / Euclid(3), CircularCircular on the circle, ManifoldFactor on SE(2)
enum { NBP_CLS_LIN2 = 1, NBP_CLS_LIN3 = 3, NBP_CLS_CIRC = 4, NBP_CLS_SE2 = 5 };
#define NBP_CLS_SIMPLE 256
static int proposals_uniform_class(const nbp_proposal_desc *d, int n) {
  if (n <= 0) return 0;
  const int M = d[0].manifold;
  const int cls = M == NBP_EUCLID2 ? NBP_CLS_LIN2 : (M == NBP_EUCLID3 ? NBP_CLS_LIN3 : (M == NBP_CIRCULAR ? NBP_CLS_CIRC : (M == NBP_SE2 ? NBP_CLS_SE2 : 0)));
  const int want = M == NBP_CIRCULAR ? NBP_F_CIRCULAR : (M == NBP_SE2 ? NBP_F_SE2 : NBP_F_LINREL);
  if (!cls) return 0;
  // "simple" (bit 8, NBP_CLS_SIMPLE): every particle of every proposal on the factor's one hypothesis -- no multihypo, no
  // nullhypo, no injected hypothesis indices, binary relatives: what the one-wave-per-proposal kernels are written for
  bool simple = true;
  for (int i = 0; i < n; i++) {
    if (d[i].manifold != M) return 0;
    const int k = d[i].factor_kind;
    if (d[i].partial_mask) return 0;  // partial priors and partial relatives run the generic kernel
    if (d[i].has_multihypo || d[i].nullhypo != 0.0 || d[i].mhidx_in >= 0) simple = false;
    if (k == NBP_F_PRIOR || k == NBP_F_MSGPRIOR || k == NBP_F_PASSTHROUGH) continue;
    if (k != want) return 0;
    if (d[i].nvars != 2) simple = false;
  }
  // (a batch of priors / message priors alone runs its manifold's instance as well)
  return cls | (simple ? NBP_CLS_SIMPLE : 0);
}
// simple Euclid(2) batches at N = 200, us per launch (profiles/r13_proposal_split_geometry.txt): 488 proposals 162 workgroup /
// 171 split, 550: 172 / 176, 700: 200 / 188; 3200: 528 split / 604 one wave, 4000: 656 / 630 -- the crossovers, rounded
#define NBP_SPLIT_MIN_DEFAULT 600
#define NBP_WAVE_MIN_LIN2_DEFAULT 3500
// What a proposal launch runs, decided in one place (launch_proposals; nbp_plan_proposals): the geometry (0: a workgroup per
// proposal, 1: one wave, 2: two waves), the grid, the workgroup, the LDS and the kernel's name.  `cls` as
// proposals_uniform_class gives it.
struct nbp_proposal_plan {
  int geometry = 0, blocks = 0, threads = 0;
  size_t lds = 0;
  const char *name = "";
};
static nbp_proposal_plan proposal_plan(const nbp_ctx *c, int n, int cls) {
  nbp_proposal_plan q;
  const bool simple = (cls & NBP_CLS_SIMPLE) != 0;
  cls &= NBP_CLS_SIMPLE - 1;
  // chip-filling launches of simple Euclidean batches: one wave per proposal, no workgroup barrier (nbp_kernels.h,
  // proposal_wave_body); rows of up to five waves (N <= 320)
  const int wave_min = c->prop_wave_min >= 0 ? c->prop_wave_min : (cls == NBP_CLS_LIN2 ? NBP_WAVE_MIN_LIN2_DEFAULT : (c->N > 256 ? 1500 : (1 << 30)));
  if (simple && n >= wave_min && (cls == NBP_CLS_LIN2 || cls == NBP_CLS_LIN3) && c->N <= (cls == NBP_CLS_LIN2 ? 256 : 320)) {
    q.geometry = 1;
    q.blocks = (n + NBP_PW_WAVES - 1) / NBP_PW_WAVES;
    q.threads = 64 * NBP_PW_WAVES;
    q.lds = nbp_proposal_wave_lds_bytes(c->N, cls == NBP_CLS_LIN2 ? 2 : 3);
    q.name = cls == NBP_CLS_LIN2 ? "nbp_proposal_wave_kernel_lin2" : (c->N <= 256 ? "nbp_proposal_wave_kernel_lin3" : "nbp_proposal_wave_kernel_lin3n5");
    return q;
  }
  // between the two: two waves per proposal, each owning every second chunk of 64 particles (proposal_split_body)
  const int split_min = c->prop_split_min >= 0 ? c->prop_split_min : NBP_SPLIT_MIN_DEFAULT;
  if (simple && cls == NBP_CLS_LIN2 && c->N <= 256 && n >= split_min) {
    q.geometry = 2;
    q.blocks = n;
    q.threads = 64 * NBP_PS_W;
    q.lds = nbp_proposal_split_lds_bytes(c->N, 2);
    q.name = "nbp_proposal_split_kernel_lin2";
    return q;
  }
  q.blocks = n;
  q.threads = c->Npad;
  q.lds = nbp_proposal_lds_bytes(c->N);
  q.name = cls == NBP_CLS_LIN2 ? "nbp_proposal_kernel_lin2" : (cls == NBP_CLS_LIN3 ? "nbp_proposal_kernel_lin3" : (cls == NBP_CLS_CIRC ? "nbp_proposal_kernel_circ" :
           (cls == NBP_CLS_SE2 ? "nbp_proposal_kernel_se2" : "nbp_proposal_kernel")));
  return q;
}
static nbp_status launch_proposals(nbp_ctx *c, const nbp_launch_env &env, const nbp_proposal_desc *dev, int n, int cls = 0) {
  if (n <= 0) return NBP_OK;
  nbp_status rc = tic(c, c->ev[0]);
  if (rc) return rc;
  (void)hipGetLastError();  // clear stale, unrelated errors
  const nbp_proposal_plan q = proposal_plan(c, n, cls);
  cls &= NBP_CLS_SIMPLE - 1;
  if (q.geometry == 1) {
    auto *wk = cls == NBP_CLS_LIN2 ? nbp_proposal_wave_kernel_lin2 : (c->N <= 256 ? nbp_proposal_wave_kernel_lin3 : nbp_proposal_wave_kernel_lin3n5);
    hipLaunchKernelGGL(wk, dim3(q.blocks), dim3(q.threads), q.lds, env.stream, dev, n, c->arena, c->N, c->S, c->side, c->counters);
  } else if (q.geometry == 2) {
    hipLaunchKernelGGL(nbp_proposal_split_kernel_lin2, dim3(q.blocks), dim3(q.threads), q.lds, env.stream, dev, c->arena, c->N, c->S, c->side, c->counters);
  } else {
    auto *kern = cls == NBP_CLS_LIN2 ? nbp_proposal_kernel_lin2 : (cls == NBP_CLS_LIN3 ? nbp_proposal_kernel_lin3 : (cls == NBP_CLS_CIRC ? nbp_proposal_kernel_circ :
                 (cls == NBP_CLS_SE2 ? nbp_proposal_kernel_se2 : nbp_proposal_kernel)));
    hipLaunchKernelGGL(kern, dim3(q.blocks), dim3(q.threads), q.lds, env.stream, dev, c->arena, c->N, c->Npad, c->S, c->side, c->counters);
  }
  HIPCHK(hipGetLastError());
  c->prop_launches[q.geometry]++;
  return toc(c, c->ev[0]);
}
// room for the KD builds of nprod products in the environment's workspace; outside a round the context's workspace grows
// (and `env` follows it)
static nbp_status ensure_ws(nbp_ctx *c, nbp_launch_env &env, int nprod, int kdF) {
  const size_t need = (size_t)nprod * (size_t)kdF * nbp_kd_ws_doubles(c->N);
  if (need <= env.ws_doubles) return NBP_OK;
  // a half of a two-stream round may hold an INTERIOR pointer of the workspace (the second half's share): never freed or
  // re-allocated here -- the round is sized at finalize, a shortfall now is a planning error, not a reason to grow
  if (env.geom_n) return fail(NBP_ERR_RANGE, "KD workspace too small inside a two-stream round (sized at nbp_program_finalize)");
  if (env.lane) return fail(NBP_ERR_RANGE, "KD workspace too small for a lane of a program (sized at nbp_program_finalize)");
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->ws) HIPCHK(hipFree(c->ws));
  c->ws = nullptr;
  c->ws_doubles = 0;
  c->ws_gen++;  // captured graphs hold the old pointer as a kernel argument: they are re-captured before their next replay
  const size_t grown = need + need / 4 + 16 * nbp_kd_ws_doubles(c->N);
  HIPCHK(hipMalloc(&c->ws, grown * 8));
  c->ws_doubles = grown;
  env.ws = c->ws;
  env.ws_doubles = c->ws_doubles;
  return NBP_OK;
}
static nbp_status ensure_gstats(nbp_ctx *c, size_t need) {
  if (need <= c->gstats_doubles) return NBP_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->gstats) HIPCHK(hipFree(c->gstats));
  c->gstats = nullptr;
  c->ws_gen++;
  c->gstats_doubles = need + need / 4;
  HIPCHK(hipMalloc(&c->gstats, c->gstats_doubles * 8));
  return NBP_OK;
}

// A list of bandwidth fits (manikde!): one (slot, manifold) per fit, in launch order.  The kernels read a list as
// [slots | manifolds] (append_fits lays it out; `off` = where, in the program blob).
struct nbp_fits {
  struct fit { int32_t slot, mani; };
  std::vector<fit> v;
  size_t off = 0;
  void push(int32_t slot, int32_t mani) { v.push_back({slot, mani}); }
  void clear() { v.clear(); }
  bool empty() const { return v.empty(); }
  int size() const { return (int)v.size(); }
  bool has(int32_t slot) const { return std::any_of(v.begin(), v.end(), [&](const fit &f) { return f.slot == slot; }); }
  void drop(int32_t slot) { v.erase(std::remove_if(v.begin(), v.end(), [&](const fit &f) { return f.slot == slot; }), v.end()); }
  void rename(int32_t a, int32_t b) { for (fit &f : v) if (f.slot == a) f.slot = b; }
  void dedup() {  // one fit per slot: the first
    for (size_t q = 0; q < v.size(); q++)
      v.erase(std::remove_if(v.begin() + q + 1, v.end(), [&](const fit &f) { return f.slot == v[q].slot; }), v.end());
  }
  // fitted coordinates (sum of the manifold dimensions) of fits [from, from + n)
  int coords(int from = 0, int n = -1) const {
    int cds = 0;
    for (int i = from; i < (n < 0 ? size() : from + n); i++) cds += manifold_dim_h(v[i].mani);
    return cds;
  }
};
// fits [from, from + n) of a list as a launch takes them: device pointers into the uploaded copy at `base`
struct nbp_fits_dev { const int32_t *slots = nullptr, *manis = nullptr; int n = 0, coords = 0; };
static nbp_fits_dev fits_dev(const nbp_fits &f, const void *base, int from = 0, int n = -1) {
  if (n < 0) n = f.size() - from;
  const int32_t *s = (const int32_t *)((const char *)base + f.off);
  return {s + from, s + f.size() + from, n, f.coords(from, n)};
}
// the list behind `blob`, 64-byte aligned: slots, manifolds, `tail` spare bytes
static void append_fits(std::vector<char> &blob, nbp_fits &f, size_t tail = 0) {
  f.off = (blob.size() + 63) & ~(size_t)63;
  blob.resize(f.off + (size_t)f.size() * 8 + tail);
  int32_t *w = (int32_t *)(blob.data() + f.off);
  for (int i = 0; i < f.size(); i++) { w[i] = f.v[i].slot; w[f.size() + i] = f.v[i].mani; }
}

// ---- fit launches ----
// Helper rows per particle for the LCV / KD launches: P = 4 (1024-lane workgroups) minimises the
// latency of a single fit when the launch cannot fill the chip; P = 2 (512 lanes) lets four
// workgroups share a CU so that the barrier/combine phases of one overlap the pair loop of the
// others when there are many fits (throughput mode).
// throughput-mode fits whose workgroup is 4k + 1 waves (N = 257 .. 320: config 5's N = 300) run the five-waves-per-SIMD
// instances of the fit kernels: four such workgroups per CU, five waves on every SIMD, instead of three (nbp_kernels.h)
// Speculation: latency mode, a handful of fits and the rest of the chip idle -> 3 workgroups per fitted coordinate (two
// iterations per rendezvous), 7 (three) where the whole launch is still resident at once (NBP_SPEC_MAXBLOCKS above).
// One plan for the fits of a prep launch (beside the KD builds of nprod products of up to kdF densities) and of a plain
// bandwidth launch (nprod = 0); each keeps its own grid shape, which its kernel indexes by.
struct nbp_fit_plan {
  int P = 1;          // helper rows per particle
  int depth = 0;      // speculation: 0 (none), 2 or 3 iterations per rendezvous = KS workgroups per fitted coordinate
  int KS = 1;
  bool w5 = false;    // the five-wave instance (plain launches only)
  int threads = 0;    // workgroup size
  size_t lds = 0;     // dynamic LDS bytes
};
static nbp_fit_plan fit_plan(const nbp_ctx *c, const nbp_launch_env &env, int nbw, int coords, int nprod = 0, int kdF = 0) {
  nbp_fit_plan f;
  const int nkd = nprod * kdF;  // KD-build workgroups
  const int nblocks = env.geom_blocks ? env.geom_blocks : 2 * nbw + 2 * nprod;
  f.P = c->P;
  if (nblocks > c->lcv_p2_min && f.P > 2) f.P = 2;
  if (nblocks > c->lcv_p1_min) f.P = 1;
  if (c->spec_on && nbw > 0 && nbw <= NBP_SPEC_MAXJOBS && !env.geom_n) {
    if (c->spec_depth3 && coords * 7 + nkd <= NBP_SPEC_MAXBLOCKS) f.depth = 3;
    else if (coords * 3 + nkd <= NBP_SPEC_MAXBLOCKS) f.depth = 2;
  }
  f.KS = f.depth ? (1 << f.depth) - 1 : 1;
  f.w5 = !f.depth && c->fit_w5 && f.P == 1 && ((c->Npad >> 6) & 3) == 1 && c->Npad > 64;
  f.threads = f.P * c->Npad;
  if (nbw > 0) f.lds = nbp_bandwidth_lds_bytes(c->N, c->Npad, f.P);
  if (nkd > 0) f.lds = std::max(f.lds, nbp_kd_lds_bytes(3, c->N, c->Npad, f.P));
  return f;
}
// a fit plan as nbp_plan_fits / nbp_last_plans report it (`prep`: the launch is launch_prep's)
static nbp_fit_plan_rec fit_plan_rec(const nbp_ctx *c, const nbp_launch_env &env, int nbw, int coords, int nprod, int kdF, bool prep, const nbp_fit_plan &f) {
  nbp_fit_plan_rec r{};
  r.status = NBP_OK;
  r.P = f.P; r.depth = f.depth; r.KS = f.KS; r.w5 = f.w5; r.threads = f.threads; r.prep = prep;
  r.N = c->N; r.fits = nbw; r.coords = coords; r.products = nprod; r.kdF = kdF; r.geom_blocks = env.geom_blocks;
  r.lds = (int64_t)f.lds;
  snprintf(r.kernel, sizeof(r.kernel), "%s%s", prep ? "nbp_prep_kernel" : "nbp_bandwidth_kernel", f.depth == 3 ? "_spec<3>" : (f.depth == 2 ? "_spec<2>" : (f.w5 ? "_w5" : "")));
  return r;
}

// ---- product launches ----
// Geometry: HL helper lanes per sample (64/HL samples per wave), workgroups of `wpb` waves, grid.y = G workgroups per product.
// Latency mode (the launch cannot fill the chip): HL = 32 for fewer than 16 products, else HL = 8, with several small
// workgroups per product (below NBP_PRODUCT_HL2_MIN products); throughput mode: HL = 2 so that one workgroup covers all samples
// and the node statistics of a product are computed once.
// Latency geometries: workgroups of FOUR waves (one per SIMD of their CU; six until round 4: config 3's products 25.9 -> 24.4 ms,
// config 2's 7.93 -> 7.77, config 4's 110.6 -> 107.8; two / three / five waves measured worse than four)
static const int NBP_PRODUCT_LAT_WAVES = 4;
// Throughput geometries: workgroups of EIGHT waves when the even split is not a multiple of four (N = 300 at two helper
// lanes: 10 waves of samples -> two workgroups of 8 instead of two of 5; N = 200: 7 -> 8).  A workgroup whose waves do not
// divide over the four SIMDs leaves one of them a wave short and makes its own waves wait for each other at the level
// barriers; the idle waves of the rounder workgroup have no samples and cost a few barriers.  Config 5: products 174.9 ->
// 164.2 ms per solve; config 2: unchanged (7.91 / 7.92 ms).  Workgroups of four (more of them per product, every one staging
// the node statistics again) measured worse: 215.7 ms.
static const int NBP_PRODUCT_THR_WAVES = 8;
// The circle: workgroups of FOUR waves in the throughput geometries too.  Its instances hold 162 VGPRs = three waves per SIMD =
// twelve wave slots per CU, of which one workgroup of eight leaves four empty and three workgroups of four none; the second
// staging per product is cheap in one dimension.  Config 3: products 24.4 -> 22.8 ms, 52.8 -> 51.3 ms per solve.  (SE(2), two
// waves per SIMD and a costly staging: 107 -> 126 ms -- it keeps eight.)
static const int NBP_PRODUCT_CIRC_WAVES = 4;
// A product whose samples need more than eight waves: ONE workgroup of up to sixteen (a multiple of four) where the kernel takes
// it -- the Euclidean instances, NBP_PROD_WIDE in nbp_kernels.h -- instead of a full workgroup and a nearly empty one, each
// staging the node statistics (N = 300 at two helper lanes: ten waves of samples; config 5's products 162 -> 122 ms per solve).
// (two helper lanes only, i.e. launches that fill the chip: a launch of 80-191 products at four helper lanes leaves CUs idle, and
//  there two workgroups per product on two CUs beat one on one -- config 2: 18.34 against 18.58 ms)
static const int NBP_PRODUCT_WIDE_WAVES = 16;
// LDS budget of a product workgroup: beyond it the node statistics live in global memory ("big")
static const size_t NBP_PRODUCT_LDS_CAP = 150 * 1024;
// chunks per helper range of a throughput launch: as many as the LDS takes while two workgroups still share a CU (80 KB each)
static const size_t NBP_PRODUCT_NCH_LDS = 80 * 1024;
// resident levels: where two workgroups of the launch still fit a CU's 160 KB
static const size_t NBP_PRODUCT_ALL_LEVELS_LDS = 76 * 1024;
// the `_w1` instances: launches of at most this many workgroups (= CUs of the chip)
static const long NBP_PRODUCT_W1_BLOCKS = 256;

// `mani`: the manifold of a single-manifold batch (0: mixed; < 0: size for the widest workgroup any kernel takes)
// `lanes`: 0, or the helper lanes per sample to take whatever the batch size says
static void product_geometry(const nbp_ctx *c, const nbp_launch_env &env, int n, int *HL, int *wpb, int *G, int mani, int lanes = 0) {
  if (env.geom_n) n = env.geom_n;  // one half of a two-stream round: the geometry of the whole batch
  *HL = lanes ? lanes : (n >= c->prod_hl2_min ? 2 : (n >= 16 ? 8 : 32));
  const int SW = 64 / *HL, waves = (c->N + SW - 1) / SW, cap = (*HL >= 8) ? NBP_PRODUCT_LAT_WAVES : 8;
  int g = (waves + cap - 1) / cap;
  *wpb = (waves + g - 1) / g;
  *G = (waves + *wpb - 1) / *wpb;
  if (*HL <= 4 && (*wpb & 3)) {
    *wpb = NBP_PRODUCT_THR_WAVES;
    *G = (waves + *wpb - 1) / *wpb;
  }
  if (mani == NBP_CIRCULAR && *HL <= 4) {
    *wpb = NBP_PRODUCT_CIRC_WAVES;
    *G = (waves + *wpb - 1) / *wpb;
  }
  const bool wide = mani < 0 || NBP_PROD_WIDE(mani);
  if (wide && *HL == 2 && waves > 8) {
    const int g2 = (waves + NBP_PRODUCT_WIDE_WAVES - 1) / NBP_PRODUCT_WIDE_WAVES;
    *wpb = (((waves + g2 - 1) / g2) + 3) & ~3;
    *G = (waves + *wpb - 1) / *wpb;
  }
}
// the sin / cos rows of the node statistics are part of a product launch's LDS unless it runs a single-manifold throughput
// kernel of a manifold without a circular coordinate (product_kernel_uniform lays its LDS out by the same rule)
static inline bool product_lays_circ(int HL, int mani) { return HL >= 8 || !(mani == NBP_EUCLID1 || mani == NBP_EUCLID2 || mani == NBP_EUCLID3); }

// Everything a product launch of n products needs to know, decided in ONE place: the launch itself, the prep launch in front
// of it (whether the node sums are left out), the presizing of its scratch area and the two-stream guard of
// nbp_program_finalize all read this plan.  (Through round 5 the guard and the presizing decided "big" on their own and left
// the chunk sums out: a round of Euclid(3) products at N = 300 with five densities passed the guard, was pipelined, and its
// halves -- laid out by the geometry of the whole batch, whose kernels have no scratch path -- ran past the LDS the launch
// had allocated.)
struct nbp_product_plan {
  int HL = 0, wpb = 0, G = 0;   // product_geometry
  bool big = false;             // the node statistics live in global memory (`gstats` doubles of it)
  bool xs = false;              // node sums from the sorted coordinates (the _xs kernels): the prep launch leaves them out
  bool circ = false;            // the LDS holds the sin / cos rows (product_lays_circ)
  int nch = 0;                  // chunks per helper range whose sums live in LDS (throughput geometry; 0: none)
  bool all_levels = false;      // the statistics of every level staged at once (NBP_PROD_ALL_LEVELS)
  bool w1 = false;              // a `_w1` kernel
  size_t lds = 0, gstats = 0;   // dynamic LDS bytes per workgroup; doubles of the global statistics area (big only)
  nbp_product_fn fn = nullptr;  // from NBP_PRODUCT_KERNELS (nullptr: the table has none for this plan)
  int row = -1;                 // its row there
};
// `maxFD` encodes the largest (F, D) of the batch as F*4 + D; `mani` as for product_geometry
static nbp_product_plan product_plan(const nbp_ctx *c, const nbp_launch_env &env, int n, int maxFD, int mani) {
  nbp_product_plan p;
  const int F = maxFD / 4, D = maxFD % 4;
  product_geometry(c, env, n, &p.HL, &p.wpb, &p.G, mani);
  // big: the statistics do not fit with the chunk sums the throughput geometries keep in LDS (two chunks per lane at least)
  p.big = nbp_product_lds_bytes(F, D, c->N, p.wpb * 64 / p.HL, false, p.HL <= 4 ? (size_t)2 * 2 * p.wpb * 64 : 0,
                                product_lays_circ(p.HL, mani)) > NBP_PRODUCT_LDS_CAP;
  // many densities: small sample groups keep the label table in LDS, and only the generic kernels of EIGHT helper lanes have the
  // scratch path.  (Asked for by lanes, not by a batch size of 16: under NBP_PRODUCT_HL2_MIN <= 16 that size is a throughput
  //  batch, the plan stayed at two helper lanes and a kernel without the scratch path ran past its LDS -- DESIGN.md 8.)
  if (p.big && p.HL != 8) product_geometry(c, env, 16, &p.HL, &p.wpb, &p.G, 0, 8);
  const int TB = p.wpb * 64, SPB = TB / p.HL;
  p.circ = product_lays_circ(p.HL, mani);
  // The launch takes the node sums from the sorted coordinates itself (4 KB instead of 33 KB of KD workspace per density
  // through HBM) when the batch runs a single-manifold throughput kernel and every product has at most NBP_FUSED_MAXF densities
  p.xs = c->prod_xs && mani > 0 && n > 0 && !p.big && p.HL <= 4 && F <= NBP_FUSED_MAXF &&
         nbp_product_lds_bytes(F, D, c->N, SPB, false, (size_t)2 * 2 * TB, p.circ) + 8 + nbp_product_xs_doubles(F, D, c->N) * 8 <=
             NBP_PRODUCT_LDS_CAP;
  const size_t xsb = p.xs ? 8 + nbp_product_xs_doubles(F, D, c->N) * 8 : 0;
  // chunks per helper range of a throughput launch (pass 2 of a draw rescans ONE chunk): as many as the LDS takes while two
  // workgroups still share a CU, else as many as one workgroup's budget takes
  if (p.HL <= 4 && !p.big) {
    auto lds_for = [&](int k) { return nbp_product_lds_bytes(F, D, c->N, SPB, false, (size_t)k * 2 * TB, p.circ) + xsb; };
    // (8 and 4 cost the same, 2 is ~5 % slower, 1 -- a range is its own chunk, pass 2 rescans all of it -- slower again; but ONE
    //  workgroup per CU costs a launch of 257 .. 512 workgroups a second generation: a mixed launch of two- and three-density
    //  products, sized by the three, took 736 us where two resident workgroups take ~600: profiles/r05_product_chunks_by_launch_size.txt)
    const int cand[4] = {8, 4, 2, 1};
    for (int k : cand)
      if (lds_for(k) <= NBP_PRODUCT_NCH_LDS) { p.nch = k; break; }
    if (!p.nch) {
      p.nch = 2;
      for (int k : cand)
        if (lds_for(k) <= NBP_PRODUCT_LDS_CAP) { p.nch = k; break; }
    }
    if (c->prod_nch >= 1 && c->prod_nch <= 15 && lds_for(c->prod_nch) <= 160 * 1024) p.nch = c->prod_nch;
  }
  p.lds = nbp_product_lds_bytes(F, D, c->N, SPB, p.big, (size_t)p.nch * 2 * TB, p.circ) + xsb;
  // resident levels (NBP_PROD_ALL_LEVELS): the statistics of every tree level staged once, no barrier between the levels
  // of the Gibbs walk
  // (the latency geometries only: a lone product saves nine round trips to the KD workspace and eighteen barriers, 126 -> 116 us;
  //  a chip-filling launch gains nothing -- NBP_PRODUCT_ALL_LEVELS_HL = 2 switches it on there too)
  if (!p.big && p.HL >= c->prod_all_levels_hl) {
    const int TOT = c->T.off[c->T.L] + c->T.cnt[c->T.L];
    // (with the chunk sums of the throughput geometries, which the kernel lays out behind the statistics: without them the
    //  experiment NBP_PRODUCT_ALL_LEVELS_HL <= 4 ran config 3's products past their LDS -- non-finite posteriors)
    const size_t lds_all = product_lds_layout(F, D, c->N, SPB, false, nullptr, nullptr, TOT, p.HL <= 4 ? (size_t)p.nch * 2 * TB : 0, p.circ) + xsb;
    if (lds_all <= NBP_PRODUCT_ALL_LEVELS_LDS) { p.lds = lds_all; p.all_levels = true; }
  }
  if (p.big) p.gstats = (size_t)n * p.G * nbp_product_gstats_doubles(F, 3, c->N);  // (the kernel's stride: largest F of the launch, D = 3)
  // the kernel: the batch's single-manifold instance where the geometry has one -- in the latency geometries only where the
  // node statistics fit the LDS (and unless NBP_NO_UNIFORM_LATENCY_PRODUCTS) -- else a generic one; `_w1` where the launch
  // has at most one workgroup (of at most four waves) per CU
  const int km = (mani > 0 && (p.HL <= 4 || (c->prod_lat_uni && !p.big))) ? mani : 0;
  p.w1 = km == 0 && p.HL >= 8 && TB <= 256 && (long)n * p.G <= NBP_PRODUCT_W1_BLOCKS && !env.geom_n;
  for (const nbp_product_kernel_row &k : NBP_PRODUCT_KERNELS)
    if (k.HL == p.HL && k.mani == km && k.xs == p.xs && k.w1 == p.w1) { p.fn = k.fn; p.row = (int)(&k - NBP_PRODUCT_KERNELS); }
  return p;
}
// what launch_products refuses of a plan (0: nothing; NBP_PLAN_REFUSED_* of nbp.h), and why
// (the halves of a two-stream round take the geometry of the whole batch, whose throughput kernels have no scratch path, and
//  share one scratch area: nbp_program_finalize pipelines no round whose products are big -- refused here should it ever)
static int product_plan_refusal(const nbp_product_plan &p, const nbp_launch_env &env, const char **why) {
  const char *w = nullptr;
  int r = 0;
  if (p.big && env.geom_n) { r = NBP_PLAN_REFUSED_BIG_IN_ROUND; w = "product: node statistics beyond the LDS inside a two-stream round"; }
  else if (p.lds > 160 * 1024) { r = NBP_PLAN_REFUSED_LDS; w = "product: too many densities for the LDS label table"; }
  else if (!p.fn) { r = NBP_PLAN_REFUSED_NO_KERNEL; w = "product: no kernel for the launch's geometry"; }
  if (why) *why = w;
  return r;
}
// a product plan as nbp_plan_products / nbp_last_plans report it
static nbp_product_plan_rec product_plan_rec(const nbp_ctx *c, const nbp_launch_env &env, int n, int maxFD, int mani, const nbp_product_plan &p) {
  nbp_product_plan_rec r{};
  r.refusal = product_plan_refusal(p, env, nullptr);
  r.status = r.refusal ? NBP_ERR_RANGE : NBP_OK;
  r.HL = p.HL; r.wpb = p.wpb; r.G = p.G; r.big = p.big; r.xs = p.xs; r.circ = p.circ; r.nch = p.nch; r.all_levels = p.all_levels; r.w1 = p.w1;
  r.row = p.row;
  if (p.row >= 0) {
    const nbp_product_kernel_row &k = NBP_PRODUCT_KERNELS[p.row];
    r.row_HL = k.HL; r.row_mani = k.mani; r.row_xs = k.xs; r.row_w1 = k.w1; r.launch_bound = k.lb;
    snprintf(r.kernel, sizeof(r.kernel), "%s", k.name);
  }
  r.N = c->N; r.n = n; r.F = maxFD / 4; r.D = maxFD % 4; r.mani = mani; r.geom_n = env.geom_n;
  r.lds = (int64_t)p.lds; r.gstats = (int64_t)p.gstats;
  return r;
}

// the rendezvous areas of the next launch of speculative fits, blanked on the launch's stream
static void blank_spec_areas(nbp_ctx *c, const nbp_launch_env &env, int jobs) {
  const int words = (int)(sizeof(nbp_spec_area) / 8) * 3 * jobs;
  hipLaunchKernelGGL(nbp_spec_blank_kernel, dim3((words + 255) / 256), dim3(256), 0, env.stream, (unsigned long long *)env_spec(c, env), words);
}

// nbp_prep_kernel: pending bandwidth fits + KD builds of this product batch, one launch (grid: 3 * KS workgroups per fit,
// then one per product and density)
static nbp_status launch_prep(nbp_ctx *c, nbp_launch_env &env, const nbp_fits_dev &bw, const nbp_product_desc *dev, int n, int maxFD, int mani = 0) {
  const int F = maxFD / 4;
  nbp_status rc = ensure_ws(c, env, n, F);
  if (rc) return rc;
  rc = tic(c, c->ev[1]);
  if (rc) return rc;
  const nbp_fit_plan f = fit_plan(c, env, bw.n, bw.coords, n, F);
  (void)hipGetLastError();
  const int kdF = F | (product_plan(c, env, n, maxFD, mani).xs ? NBP_KD_NOSTATS : 0);
  c->last_prep = fit_plan_rec(c, env, bw.n, bw.coords, n, F, true, f);
  c->last_prep.kd_nostats = (kdF & NBP_KD_NOSTATS) != 0;
  const dim3 grid(3 * bw.n * f.KS + n * F);
  if (f.depth) {
    blank_spec_areas(c, env, bw.n);
    hipLaunchKernelGGL(f.depth == 3 ? nbp_prep_kernel_spec<3> : nbp_prep_kernel_spec<2>, grid, dim3(f.threads), f.lds, env.stream, bw.slots, bw.manis,
                       bw.n, dev, n, kdF, c->arena, env.ws, c->N, c->Npad, c->S, c->T, c->counters, env_spec(c, env));
  } else
    hipLaunchKernelGGL(f.w5 ? nbp_prep_kernel_w5 : nbp_prep_kernel, grid, dim3(f.threads), f.lds, env.stream, bw.slots, bw.manis, bw.n, dev, n, kdF,
                       c->arena, env.ws, c->N, c->Npad, c->S, c->T, c->counters);
  HIPCHK(hipGetLastError());
  return toc(c, c->ev[1]);
}

// 0 unless all products with more than one density share a manifold and none has a partial input
static int products_uniform_manifold(const nbp_product_desc *d, int n) {
  int mani = -1;
  // a batch of pass-through products only (single densities: AMP returns them) runs the copy path of whichever instance:
  // the first product's manifold picks a single-manifold kernel instead of the all-manifold one (308 B of scratch per lane)
  bool multi = false;
  for (int i = 0; i < n; i++) multi |= d[i].nfactors > 1;
  if (!multi && n > 0) return d[0].manifold;
  for (int i = 0; i < n; i++) {
    if (d[i].nfactors <= 1) continue;
    for (int j = 0; j < d[i].nfactors; j++)
      if (d[i].in_partial[j]) return 0;
    if (mani == -1) mani = d[i].manifold;
    else if (mani != d[i].manifold) return 0;
  }
  return mani > 0 ? mani : 0;
}
static nbp_status launch_products(nbp_ctx *c, const nbp_launch_env &env, const nbp_product_desc *dev, int n, int maxFD, int mani = 0) {
  if (n <= 0) return NBP_OK;
  const nbp_product_plan p = product_plan(c, env, n, maxFD, mani);
  c->last_product = product_plan_rec(c, env, n, maxFD, mani, p);
  const char *why = nullptr;
  if (product_plan_refusal(p, env, &why)) return fail(NBP_ERR_RANGE, why);
  nbp_status rc = NBP_OK;
  if (p.big && env.lane == 2) {  // (beside lane 0's launches: its own area, sized at nbp_program_finalize)
    if (p.gstats > c->gstats1_doubles) return fail(NBP_ERR_RANGE, "statistics area too small for lane 1 of a program (sized at nbp_program_finalize)");
  } else if (p.big) {
    rc = ensure_gstats(c, p.gstats);
    if (rc) return rc;
  }
  rc = tic(c, c->ev[2]);
  if (rc) return rc;
  (void)hipGetLastError();
  const int flagsF = (maxFD / 4) | (p.nch << NBP_PROD_NCH_SHIFT) | (p.all_levels ? NBP_PROD_ALL_LEVELS : 0);
  hipLaunchKernelGGL(p.fn, dim3(n, p.G), dim3(p.wpb * 64), p.lds, env.stream, dev, c->arena, env.ws, flagsF,
                     p.big ? (env.lane == 2 ? c->gstats1 : c->gstats) : nullptr, c->N, c->S, c->side, c->T);
  HIPCHK(hipGetLastError());
  return toc(c, c->ev[2]);
}

// the allocations launch_prep / launch_products would make on demand for a batch of n products (outside a round: a round
// shares the workspace of its whole batch)
static nbp_status presize_products(nbp_ctx *c, int n, int maxFD, int mani = 0) {
  nbp_launch_env env = ctx_env(c);
  nbp_status rc = ensure_ws(c, env, n, maxFD / 4);
  if (rc) return rc;
  // the launch's own plan, or the widest workgroup any kernel may take (mani = -1: its larger label table decides about the
  // scratch) -- whichever asks for the scratch area gets it allocated here, outside the replayed region
  const size_t gs = std::max(product_plan(c, env, n, maxFD, mani).gstats, product_plan(c, env, n, maxFD, -1).gstats);
  if (gs) rc = ensure_gstats(c, gs);
  return rc;
}

// nbp_bandwidth_kernel: fits alone (grid: fit x coordinate x KS)
static nbp_status launch_bandwidth(nbp_ctx *c, const nbp_launch_env &env, const nbp_fits_dev &bw) {
  if (bw.n <= 0) return NBP_OK;
  nbp_status rc = tic(c, c->ev[3]);
  if (rc) return rc;
  (void)hipGetLastError();
  const nbp_fit_plan f = fit_plan(c, env, bw.n, bw.coords);
  c->last_fit = fit_plan_rec(c, env, bw.n, bw.coords, 0, 0, false, f);
  if (f.depth) {
    blank_spec_areas(c, env, bw.n);
    hipLaunchKernelGGL(f.depth == 3 ? nbp_bandwidth_kernel_spec<3> : nbp_bandwidth_kernel_spec<2>, dim3(bw.n, 3, f.KS), dim3(f.threads), f.lds, env.stream,
                       bw.slots, bw.manis, c->arena, c->N, c->Npad, c->S, c->counters, env_spec(c, env));
  } else {
    auto *kern = f.w5 ? nbp_bandwidth_kernel_w5 : nbp_bandwidth_kernel;
    if (c->debug_occupancy) {  // what the runtime says a CU can hold of this launch
      int nb = 0;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, f.threads, f.lds);
      fprintf(stderr, "[nbp] nbp_bandwidth_kernel%s: %d lanes, %zu B of LDS per workgroup: %d workgroups = %d waves per CU\n", f.w5 ? "_w5" : "",
              f.threads, f.lds, nb, nb * (f.threads / 64));
    }
    hipLaunchKernelGGL(kern, dim3(bw.n, 3), dim3(f.threads), f.lds, env.stream, bw.slots, bw.manis, c->arena, c->N, c->Npad, c->S, c->counters);
  }
  HIPCHK(hipGetLastError());
  return toc(c, c->ev[3]);
}

// The fits a batch of proposals / products queues (host side): every proposal but a pass-through and one that asks for
// none; every real product (a pass-through keeps the bandwidth of its input).  `dead`: per descriptor, fits that
// product_liveness found unread (null: none).
static bool wants_fit(const nbp_proposal_desc &d) { return !d.skip_bandwidth && d.factor_kind != NBP_F_PASSTHROUGH; }
static bool wants_fit(const nbp_product_desc &d) { return d.nfactors > 1; }
extern "C++" template <class D>
static void queue_fits(nbp_fits &q, const D *d, int n, const char *dead = nullptr) {
  for (int i = 0; i < n; i++)
    if (wants_fit(d[i]) && !(dead && dead[i])) q.push(d[i].out_slot, d[i].manifold);
}

// largest (F, D) of a product batch, encoded F*4 + D (sizes the LDS of the launch)
static int products_maxfd(const nbp_product_desc *d, int n) {
  int F = 2, D = 1;
  for (int i = 0; i < n; i++)
    if (d[i].nfactors > 1) {
      if (d[i].nfactors > F) F = d[i].nfactors;
      if (manifold_dim_h(d[i].manifold) > D) D = manifold_dim_h(d[i].manifold);
    }
  return F * 4 + D;
}
// whole slots, or (points_only: NBP_STAGE_COPY_POINTS) the points and the count, the destination's bandwidth left alone
static nbp_status launch_copies(nbp_ctx *c, const nbp_copy_desc *dev, int n, bool points_only = false, hipStream_t stream = nullptr) {
  if (n <= 0) return NBP_OK;
  (void)hipGetLastError();
  if (!stream) stream = c->stream;
  if (points_only) hipLaunchKernelGGL(nbp_copy_points_kernel, dim3(n), dim3(256), 0, stream, dev, c->arena, c->S, c->N);
  else hipLaunchKernelGGL(nbp_copy_kernel, dim3(n), dim3(256), 0, stream, dev, c->arena, c->S);
  HIPCHK(hipGetLastError());
  return NBP_OK;
}

static nbp_status stage_upload(nbp_ctx *c, const void *src, size_t bytes) {
  if (bytes > c->stage_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->stage) HIPCHK(hipFree(c->stage));
    c->stage_bytes = bytes * 2;
    HIPCHK(hipMalloc(&c->stage, c->stage_bytes));
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // the previous batch may still read the staging buffer
  HIPCHK(hipMemcpy(c->stage, src, bytes, hipMemcpyHostToDevice));
  return NBP_OK;
}

// upload [descriptors | fits] in one staging copy (fits.off = where the list lies in c->stage)
static nbp_status stage_with_fits(nbp_ctx *c, const void *descs, size_t desc_bytes, nbp_fits &fits) {
  std::vector<char> buf((const char *)descs, (const char *)descs + desc_bytes);
  append_fits(buf, fits, 8);
  return stage_upload(c, buf.data(), buf.size());
}

nbp_status nbp_run_proposals(nbp_ctx *c, const nbp_proposal_desc *descs, int32_t n) {
  if (!c || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  nbp_status rc = check_proposals(c, descs, n);
  if (rc) return rc;
  nbp_fits fits;
  queue_fits(fits, descs, n);
  rc = stage_with_fits(c, descs, sizeof(nbp_proposal_desc) * (size_t)n, fits);
  if (rc) return rc;
  rc = launch_proposals(c, ctx_env(c), (const nbp_proposal_desc *)c->stage, n, proposals_uniform_class(descs, n));
  if (rc) return rc;
  rc = launch_bandwidth(c, ctx_env(c), fits_dev(fits, c->stage));  // manikde!(M, pts), ApproxConv.jl:36-42
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

nbp_status nbp_run_products(nbp_ctx *c, const nbp_product_desc *descs, int32_t n) {
  if (!c || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  nbp_status rc = check_products(c, descs, n);
  if (rc) return rc;
  nbp_fits fits;
  queue_fits(fits, descs, n);
  rc = stage_with_fits(c, descs, sizeof(nbp_product_desc) * (size_t)n, fits);
  if (rc) return rc;
  const int maxfd = products_maxfd(descs, n), mani = products_uniform_manifold(descs, n);
  nbp_launch_env env = ctx_env(c);
  rc = launch_prep(c, env, nbp_fits_dev{}, (const nbp_product_desc *)c->stage, n, maxfd, mani);  // KD trees
  if (rc) return rc;
  rc = launch_products(c, env, (const nbp_product_desc *)c->stage, n, maxfd, mani);
  if (rc) return rc;
  rc = launch_bandwidth(c, env, fits_dev(fits, c->stage));  // rebandwidth of the product
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

static nbp_status check_deconv(nbp_ctx *c, const nbp_proposal_desc *descs, int n) {
  nbp_status rc = check_proposals(c, descs, n);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const nbp_proposal_desc &p = descs[i];
    if (p.factor_kind < NBP_F_LINREL) return fail(NBP_ERR_ARG, "deconv: relative factors only (a prior's predicted measurement is the point itself)");
    if (p.has_multihypo || p.nvars != 2) return fail(NBP_ERR_ARG, "deconv: multihypo is not supported (reference issue #467/#927)");
    if (p.partial_mask) return fail(NBP_ERR_ARG, "deconv: partial factors are not supported");
  }
  return NBP_OK;
}

static nbp_status launch_deconv(nbp_ctx *c, const nbp_proposal_desc *dev_descs, const int32_t *dev_meas, int n) {
  if (n <= 0) return NBP_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(nbp_deconv_kernel, dim3(n), dim3(c->Npad), 0, c->stream, dev_descs, dev_meas, c->arena, c->N, c->S, c->counters);
  HIPCHK(hipGetLastError());
  return NBP_OK;
}

nbp_status nbp_run_deconv(nbp_ctx *c, const nbp_proposal_desc *descs, const int32_t *meas_slots, int32_t n) {
  if (!c || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  nbp_status rc = check_deconv(c, descs, n);
  if (rc) return rc;
  // [descriptors | slot of each measurement, or -1] in one staging copy
  const size_t off = (sizeof(nbp_proposal_desc) * (size_t)n + 63) & ~(size_t)63;
  std::vector<char> buf(off + (size_t)n * 4);
  memcpy(buf.data(), descs, sizeof(nbp_proposal_desc) * (size_t)n);
  for (int i = 0; i < n; i++) {
    if (meas_slots && meas_slots[i] >= c->n_slots) return fail(NBP_ERR_RANGE, "deconv: meas_slot");
    ((int32_t *)(buf.data() + off))[i] = meas_slots ? meas_slots[i] : -1;
  }
  rc = stage_upload(c, buf.data(), buf.size());
  if (rc) return rc;
  const int32_t *ds = (const int32_t *)((char *)c->stage + off);
  rc = tic(c, c->ev[0]);
  if (rc) return rc;
  rc = launch_deconv(c, (const nbp_proposal_desc *)c->stage, ds, n);
  if (rc) return rc;
  rc = toc(c, c->ev[0]);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// ---- host-buffer entry points: one call per reference function, for callers that keep beliefs on the
// host (the Julia shim's factor / variable seams).  They stage through the first slots of the context.
nbp_status nbp_kde_bandwidth(nbp_ctx *c, int32_t manifold, const double *pts, double *bw_out) {
  if (!c || !pts || !bw_out) return fail(NBP_ERR_ARG, "null argument");
  nbp_status rc = nbp_slot_write(c, 0, manifold, pts, nullptr);
  if (rc) return rc;
  const int32_t slot = 0;
  rc = nbp_run_bandwidth(c, &slot, &manifold, 1);
  if (rc) return rc;
  std::vector<double> tmp((size_t)c->N * 6);
  return nbp_slot_read(c, 0, manifold, tmp.data(), bw_out);
}

nbp_status nbp_conv(nbp_ctx *c, const nbp_proposal_desc *tmpl, const double *const *var_pts, const double *const *var_bw,
                    const int32_t *mhidx_in, double *out_pts, double *out_bw, int32_t *out_mhidx) {
  if (!c || !tmpl || !var_pts || !out_pts) return fail(NBP_ERR_ARG, "null argument");
  nbp_proposal_desc d = *tmpl;
  const int nin = (d.factor_kind == NBP_F_MSGPRIOR || d.factor_kind == NBP_F_PASSTHROUGH) ? 2 : d.nvars;
  if (nin < 1 || nin > NBP_MAXV) return fail(NBP_ERR_RANGE, "conv: nvars");
  if (c->n_slots < nin + 1) return fail(NBP_ERR_RANGE, "conv: the context needs nvars + 1 slots");
  if ((mhidx_in || out_mhidx) && c->side_ints < 2 * c->N) return fail(NBP_ERR_RANGE, "conv: the context needs 2N side ints");
  for (int i = 0; i < nin; i++) {
    if (!var_pts[i]) return fail(NBP_ERR_ARG, "conv: null variable points");
    nbp_status rc = nbp_slot_write(c, i, d.manifold, var_pts[i], var_bw ? var_bw[i] : nullptr);
    if (rc) return rc;
    d.var_slot[i] = i;
  }
  d.out_slot = nin;
  d.mhidx_in = -1;
  d.mhidx_out = -1;
  if (mhidx_in) {
    nbp_status rc = nbp_side_write(c, 0, mhidx_in, c->N);
    if (rc) return rc;
    d.mhidx_in = 0;
  }
  if (out_mhidx) d.mhidx_out = c->N;
  d.skip_bandwidth = out_bw ? 0 : 1;
  nbp_status rc = nbp_run_proposals(c, &d, 1);
  if (rc) return rc;
  rc = nbp_slot_read(c, nin, d.manifold, out_pts, out_bw);
  if (rc) return rc;
  if (out_mhidx) rc = nbp_side_read(c, c->N, out_mhidx, c->N);
  return rc;
}

nbp_status nbp_manifold_product(nbp_ctx *c, int32_t manifold, int32_t F, const double *const *dens_pts, const double *const *dens_bw,
                                const uint8_t *partial_masks, const double *old_pts, int32_t niter, uint64_t seed,
                                double *out_pts, double *out_bw, int32_t *out_labels) {
  if (!c || !dens_pts || !dens_bw || !out_pts) return fail(NBP_ERR_ARG, "null argument");
  if (F < 1 || F > NBP_MAXF) return fail(NBP_ERR_RANGE, "product: nfactors");
  if (c->n_slots < F + 2) return fail(NBP_ERR_RANGE, "product: the context needs F + 2 slots");
  if (out_labels && c->side_ints < c->N * F) return fail(NBP_ERR_RANGE, "product: the context needs N*F side ints");
  nbp_product_desc d;
  memset(&d, 0, sizeof(d));
  d.manifold = manifold;
  d.nfactors = F;
  d.niter = niter;
  d.out_slot = F + 1;
  d.labels_out = out_labels ? 0 : -1;
  d.old_slot = -1;
  d.seed = seed;
  for (int j = 0; j < F; j++) {
    if (!dens_pts[j] || !dens_bw[j]) return fail(NBP_ERR_ARG, "product: null density");
    nbp_status rc = nbp_slot_write(c, j, manifold, dens_pts[j], dens_bw[j]);
    if (rc) return rc;
    d.in_slot[j] = j;
    d.in_partial[j] = partial_masks ? partial_masks[j] : 0;
  }
  if (old_pts) {
    nbp_status rc = nbp_slot_write(c, F, manifold, old_pts, nullptr);
    if (rc) return rc;
    d.old_slot = F;
  }
  nbp_status rc = nbp_run_products(c, &d, 1);
  if (rc) return rc;
  rc = nbp_slot_read(c, F + 1, manifold, out_pts, out_bw);
  if (rc) return rc;
  if (out_labels) rc = nbp_side_read(c, 0, out_labels, c->N * F);
  return rc;
}

nbp_status nbp_run_copies(nbp_ctx *c, const nbp_copy_desc *descs, int32_t n) {
  if (!c || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  nbp_status rc = check_copies(c, descs, n);
  if (rc) return rc;
  rc = stage_upload(c, descs, sizeof(nbp_copy_desc) * (size_t)n);
  if (rc) return rc;
  rc = launch_copies(c, (const nbp_copy_desc *)c->stage, n);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// slot copies queued on the library stream, nothing waited for (resident beliefs of the asynchronous clique seam:
// nbp_resident_copy).  The descriptors are read by the kernel from a pinned buffer of the context's pool (device-visible
// host memory: a few bytes per workgroup), freed behind the launch.  points_only: NBP_STAGE_COPY_POINTS semantics.
nbp_status nbp_run_copies_async(nbp_ctx *c, const nbp_copy_desc *descs, int32_t n, int32_t points_only) {
  if (!c || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  nbp_status rc = check_copies(c, descs, n);
  if (rc) return rc;
  nbp_ctx::pin_buf *b = pin_acquire(c, sizeof(nbp_copy_desc) * (size_t)n);
  if (!b) return fail(NBP_ERR_HIP, "pinned staging buffer");
  memcpy(b->p, descs, sizeof(nbp_copy_desc) * (size_t)n);
  rc = launch_copies(c, (const nbp_copy_desc *)b->p, n, points_only != 0);
  pin_release_behind_stream(c, b);
  return rc;
}

// ---- batches over resident beliefs -------------------------------------------------------------------------------------------
// Every nbp_run_* below is one sequence: the device selected and the columns checked (batch_check), the columns staged in
// one copy and the result scratch reserved (stage_columns), one launch (launch_checked), the results copied back and the stream
// waited for (query_fetch, scratch_layout::fetch).  The nbp_kde_* forms put their host buffers into slot 0 (and 1) first (kde_check,
// kde_write), and EVERY REFUSAL OF SUCH A FORM COMES BEFORE SLOT 0 IS TOUCHED: what the batch form refuses in an element is one function
// (grid_desc_check, credible_check, overlap_check, likelihood_check), which the host-buffer form calls on its own element before kde_write.
// the scratch of the belief queries holds at least `doubles` (called with the stream idle: stage_upload has waited)
static nbp_status query_reserve(nbp_ctx *c, size_t doubles) {
  if (doubles <= c->query_cap) return NBP_OK;
  if (c->query) HIPCHK(hipFree(c->query));
  c->query = nullptr;
  c->query_cap = 0;
  HIPCHK(hipMalloc(&c->query, sizeof(double) * doubles * 2));
  c->query_cap = doubles * 2;
  return NBP_OK;
}

struct stage_col {
  const void *p;
  size_t bytes;
};
// columns of any plain type in ONE staging copy, each starting on an 8-byte boundary, dev[k] = where column k lies on the device
// (int32 columns but for the grid descriptors: cast there); then c->query holds `scratch` doubles
// (stage_upload waits for the stream: the query scratch is free as well)
static nbp_status stage_columns(nbp_ctx *c, std::initializer_list<stage_col> cols, const int32_t **dev, size_t scratch) {
  std::vector<char> blob;
  std::vector<size_t> off;
  for (const stage_col &col : cols) {
    off.push_back(blob.size());
    blob.resize(blob.size() + (col.bytes + 7) / 8 * 8);
    if (col.bytes) memcpy(blob.data() + off.back(), col.p, col.bytes);
  }
  NBPCHK(stage_upload(c, blob.data(), blob.size()));
  for (size_t o : off) *dev++ = (const int32_t *)((const char *)c->stage + o);
  return query_reserve(c, scratch);
}

// the one copy back, and the wait for it
static nbp_status query_fetch(nbp_ctx *c, void *dst, const void *src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// The query scratch of one entry: parts in order, each `count` elements of `elem` bytes starting on a whole double, `to` where it goes
// on the host (nullptr: nowhere).  total() is what stage_columns reserves; at(c, k) is part k on the device, asked for AFTER
// stage_columns (which may move c->query); fetch() is the one copy back, from the first to the last part wanted, and the wait for it.
struct scratch_layout {
  struct part {
    size_t elem, count;
    void *to;
  };
  std::vector<part> parts;
  std::vector<size_t> off;  // in doubles; one more than parts: the total
  scratch_layout(std::initializer_list<part> ps) : parts(ps), off(1, 0) {
    for (const part &p : parts) off.push_back(off.back() + (p.elem * p.count + 7) / 8);
  }
  size_t total() const { return off.back(); }
  double *at(const nbp_ctx *c, size_t k) const { return c->query + off[k]; }
  nbp_status fetch(nbp_ctx *c) const {
    size_t first = parts.size(), last = 0;
    for (size_t k = 0; k < parts.size(); k++)
      if (parts[k].to) first = std::min(first, k), last = k;
    if (first == last) return query_fetch(c, parts[first].to, c->query + off[first], parts[first].elem * parts[first].count);  // no detour
    std::vector<double> back(off[last + 1] - off[first]);
    NBPCHK(query_fetch(c, back.data(), c->query + off[first], sizeof(double) * back.size()));
    for (size_t k = first; k <= last; k++)
      if (parts[k].to) memcpy(parts[k].to, back.data() + (off[k] - off[first]), parts[k].elem * parts[k].count);
    return NBP_OK;
  }
  // fetch() for a layout whose parts from `big` on are large (grids): those go straight into the caller's buffers -- a staging vector
  // of their size costs more than the kernel (profiles/marginal_grid_kernel.txt, profiles/scene_grid.txt) -- and the small parts
  // before them come back in one copy; one wait for all of it
  nbp_status fetch_split(nbp_ctx *c, size_t big) const {
    for (size_t k = big; k < parts.size(); k++)
      if (parts[k].to && parts[k].count)
        HIPCHK(hipMemcpyAsync(parts[k].to, c->query + off[k], parts[k].elem * parts[k].count, hipMemcpyDeviceToHost, c->stream));
    size_t first = big, last = 0;
    for (size_t k = 0; k < big; k++)
      if (parts[k].to && parts[k].count) first = std::min(first, k), last = k;
    if (first == big) {
      HIPCHK(hipStreamSynchronize(c->stream));
      return NBP_OK;
    }
    std::vector<double> back(off[last + 1] - off[first]);
    NBPCHK(query_fetch(c, back.data(), c->query + off[first], sizeof(double) * back.size()));
    for (size_t k = first; k <= last; k++)
      if (parts[k].to) memcpy(parts[k].to, back.data() + (off[k] - off[first]), parts[k].elem * parts[k].count);
    return NBP_OK;
  }
};

// Host-buffer forms: the beliefs go through slot 0 (and slot 1), which they clobber.  bw == nullptr: the bandwidth plays no part
// in the query, the slot carries ones.
struct host_belief {
  const double *pts;
  int32_t n;
  const double *bw;
};
static nbp_status kde_check(const nbp_ctx *c, const char *who, int32_t manifold, std::initializer_list<host_belief> bels) {
  if (!manifold_ok(manifold)) return fail(NBP_ERR_ARG, std::string(who) + ": unknown manifold");
  for (const host_belief &b : bels)
    if (b.n < 1) return fail(NBP_ERR_ARG, std::string(who) + ": a belief holds at least one point");
  if (bels.size() == 2 && c->n_slots < 2) return fail(NBP_ERR_RANGE, std::string(who) + ": the context needs two slots");
  return NBP_OK;
}
static nbp_status kde_write(nbp_ctx *c, int32_t manifold, std::initializer_list<host_belief> bels) {
  const double ones[NBP_MAXD] = {1.0, 1.0, 1.0};
  int32_t slot = 0;
  for (const host_belief &b : bels)
    if (b.pts) NBPCHK(nbp_belief_write(c, slot++, manifold, b.pts, b.n, b.bw ? b.bw : ones, nullptr));  // (no points: a role a unary factor lacks)
  return NBP_OK;
}
static nbp_status kde_stage(nbp_ctx *c, const char *who, int32_t manifold, std::initializer_list<host_belief> bels) {
  NBPCHK(kde_check(c, who, manifold, bels));
  return kde_write(c, manifold, bels);
}

nbp_status nbp_run_bandwidth(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n) {
  if (!c || ((!slots || !manifolds) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "bandwidth", {slots}, manifolds, n, no_refusal));
  nbp_fits fits;
  for (int i = 0; i < n; i++) fits.push(slots[i], manifolds[i]);
  NBPCHK(stage_with_fits(c, nullptr, 0, fits));
  NBPCHK(launch_bandwidth(c, ctx_env(c), fits_dev(fits, c->stage)));
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// calcPPE (FGOSUtils.jl:237-275) of resident beliefs: one workgroup per belief (nbp_ppe.h), one copy back
nbp_status nbp_run_ppe(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, double *mean_out, double *max_out,
                       int32_t *max_index_out) {
  if (!c || ((!slots || !manifolds || !mean_out || !max_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "ppe", {slots}, manifolds, n, no_refusal));
  static_assert(sizeof(nbp_ppe_rec) % sizeof(double) == 0, "nbp_ppe_rec fills whole doubles of the query scratch");
  std::vector<nbp_ppe_rec> rec((size_t)n);
  const scratch_layout q{{sizeof(nbp_ppe_rec), (size_t)n, rec.data()}};
  const int32_t *d[2];
  NBPCHK(stage_columns(c, {{slots, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_ppe_kernel, n, c->Npad, nbp_ppe_lds_bytes(c->N), d[0], d[1], c->arena, c->N, c->S, (nbp_ppe_rec *)q.at(c, 0)));
  NBPCHK(q.fetch(c));
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < NBP_MAXD; k++) {
      mean_out[(size_t)i * NBP_MAXD + k] = rec[i].mean[k];
      max_out[(size_t)i * NBP_MAXD + k] = rec[i].max[k];
    }
    if (max_index_out) max_index_out[i] = rec[i].max_index;
  }
  return NBP_OK;
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_bandwidth
nbp_status nbp_kde_ppe(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, double *mean_out,
                       double *max_out, int32_t *max_index_out) {
  if (!c || !pts || !bw || !mean_out || !max_out) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_stage(c, "ppe", manifold, {{pts, n_pts, bw}}));
  const int32_t slot = 0;
  double mean3[NBP_MAXD], max3[NBP_MAXD];
  NBPCHK(nbp_run_ppe(c, &slot, &manifold, 1, mean3, max3, max_index_out));
  for (int k = 0; k < manifold_dim_h(manifold); k++) {
    mean_out[k] = mean3[k];
    max_out[k] = max3[k];
  }
  return NBP_OK;
}

// The launch of both point-density forms, behind their argument checks: one workgroup per tile of at most NBP_QUERY_TILE queries of
// one belief, one copy each way.  masks == nullptr: nbp_eval_kernel; else its masked instance.
static nbp_status run_point_density(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                    const int32_t *q_first, const double *queries, double *dens_out) {
  const size_t Q = (size_t)q_first[n];
  if (Q == 0) return NBP_OK;
  if (!queries || !dens_out) return fail(NBP_ERR_ARG, "null argument");
  std::vector<int32_t> tiles;  // (belief of the batch, first query, number of queries <= NBP_QUERY_TILE)
  for (int i = 0; i < n; i++)
    for (int32_t q = q_first[i]; q < q_first[i + 1]; q += NBP_QUERY_TILE) {
      tiles.push_back(i);
      tiles.push_back(q);
      tiles.push_back(std::min<int32_t>(NBP_QUERY_TILE, q_first[i + 1] - q));
    }
  const int32_t *d[4];
  NBPCHK(stage_columns(c, {{slots, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}, {masks, masks ? 4 * (size_t)n : 0}, {tiles.data(), 4 * tiles.size()}},
                                d, Q * (NBP_MAXD + 1)));
  double *dq = c->query, *dd = c->query + Q * NBP_MAXD;
  HIPCHK(hipMemcpyAsync(dq, queries, sizeof(double) * Q * NBP_MAXD, hipMemcpyHostToDevice, c->stream));
  const size_t n_tiles = tiles.size() / 3, lds = nbp_eval_lds_bytes(c->N);
  NBPCHK(masks ? launch_checked(c, nbp_eval_marginal_kernel, n_tiles, NBP_QUERY_TILE, lds, d[3], d[0], d[1], d[2], c->arena, c->N, c->S, dq, dd)
             : launch_checked(c, nbp_eval_kernel, n_tiles, NBP_QUERY_TILE, lds, d[3], d[0], d[1], c->arena, c->N, c->S, dq, dd));
  return query_fetch(c, dens_out, dd, sizeof(double) * Q);
}

// getBelief(fg, :x)(pts) for beliefs resident in slots: the density of each belief's KDE at its own run of query points
// (nbp_query.h)
nbp_status nbp_run_evaluate(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, const int32_t *q_first,
                            const double *queries, double *dens_out) {
  if (!c || ((!slots || !manifolds || !q_first) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  if (q_first[0] != 0) return fail(NBP_ERR_ARG, "evaluate: q_first[0] must be 0");
  NBPCHK(batch_check(c, "evaluate", {slots}, manifolds, n, [&](int i) {
    return q_first[i + 1] < q_first[i] ? refusal{NBP_ERR_ARG, "q_first must not decrease"} : refusal{NBP_OK, nullptr};
  }));
  return run_point_density(c, slots, manifolds, nullptr, n, q_first, queries, dens_out);
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_ppe
nbp_status nbp_kde_evaluate(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, const double *queries,
                            int32_t nq, double *dens_out) {
  if (!c || !pts || !bw || ((!queries || !dens_out) && nq > 0)) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_check(c, "evaluate", manifold, {{pts, n_pts, bw}}));
  if (nq < 0) return fail(NBP_ERR_ARG, "evaluate: nq < 0");
  NBPCHK(kde_write(c, manifold, {{pts, n_pts, bw}}));
  const int32_t slot = 0, q_first[2] = {0, nq};
  return nbp_run_evaluate(c, &slot, &manifold, 1, q_first, queries, dens_out);
}

// ---- marginal densities (nbp_marginal.h) ---------------------------------------------------------------------------------------
// One descriptor of nbp_run_marginal_grid: NBP_OK and its number of grid points, or the refusal (nothing has been launched)
static nbp_status grid_desc_check(const nbp_ctx *c, const nbp_grid_desc &g, int i, int64_t *points) {
  const std::string who = "marginal grid: descriptor " + std::to_string(i) + ": ";
  if (g.slot < 0 || g.slot >= c->n_slots) return fail(NBP_ERR_RANGE, who + "slot out of range");
  if (!manifold_ok(g.manifold)) return fail(NBP_ERR_ARG, who + "unknown manifold");
  if (g.flags & ~NBP_GRID_AUTO_EXTENT) return fail(NBP_ERR_ARG, who + "unknown flag");
  const int D = manifold_dim_h(g.manifold), axes = g.dims[1] == -1 ? 1 : 2;
  const bool autoext = g.flags & NBP_GRID_AUTO_EXTENT;
  int64_t pts = 1;
  for (int a = 0; a < axes; a++) {
    if (g.dims[a] < 0 || g.dims[a] >= D) return fail(NBP_ERR_RANGE, who + "coordinate outside the manifold");
    if (a == 1 && g.dims[1] == g.dims[0]) return fail(NBP_ERR_RANGE, who + "repeated coordinate");
    if (g.n[a] < 1 || g.n[a] > NBP_GRID_MAX) return fail(NBP_ERR_RANGE, who + "n outside 1 .. " + std::to_string(NBP_GRID_MAX));
    if (autoext && !manifold_circ_h(g.manifold, g.dims[a]) && g.n[a] < 2) return fail(NBP_ERR_RANGE, who + "automatic extent of a Euclidean axis needs n >= 2");
    if (!autoext && !(std::isfinite(g.lo[a]) && std::isfinite(g.step[a]))) return fail(NBP_ERR_RANGE, who + "lo / step not finite");
    pts *= g.n[a];
  }
  if (autoext && !std::isfinite(g.margin)) return fail(NBP_ERR_RANGE, who + "margin not finite");
  *points = pts;
  return NBP_OK;
}

// p_K of resident beliefs on regular grids: one workgroup per tile of one descriptor's grid (nbp_marginal.h); the descriptors, the
// offsets and the tile table go up in one staging copy, the grids come back in one copy (the extents, 32 bytes a descriptor, in a
// second one where the caller asks for them)
nbp_status nbp_run_marginal_grid(nbp_ctx *c, const nbp_grid_desc *descs, int32_t n, const int32_t *first, double *out,
                                 double *extent_out) {
  if (!c || ((!descs || !first) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  if (first[0] != 0) return fail(NBP_ERR_RANGE, "marginal grid: descriptor 0: first[0] must be 0");
  std::vector<int32_t> tiles;
  for (int i = 0; i < n; i++) {
    int64_t pts = 0;
    NBPCHK(grid_desc_check(c, descs[i], i, &pts));
    if ((int64_t)first[i + 1] - (int64_t)first[i] != pts)
      return fail(NBP_ERR_RANGE, "marginal grid: descriptor " + std::to_string(i) + ": offsets do not match the grid size");
    const bool two = descs[i].dims[1] != -1;
    const int t0 = two ? NBP_GRID_TILE : NBP_GRID_TILE1;
    for (int32_t k0 = 0; k0 < descs[i].n[0]; k0 += t0)
      for (int32_t k1 = 0; k1 < (two ? descs[i].n[1] : 1); k1 += NBP_GRID_TILE) {
        tiles.push_back(i);
        tiles.push_back(k0);
        tiles.push_back(k1);
      }
  }
  if (!out) return fail(NBP_ERR_ARG, "null argument");
  const size_t total = (size_t)first[n];
  // staging: descriptors | first | tiles
  const int32_t *d[3];
  NBPCHK(stage_columns(c, {{descs, sizeof(nbp_grid_desc) * (size_t)n}, {first, 4 * ((size_t)n + 1)}, {tiles.data(), 4 * tiles.size()}}, d,
                                total + 4 * (size_t)n));
  double *dgrid = c->query, *dext = c->query + total;
  NBPCHK(launch_checked(c, nbp_marginal_grid_kernel, tiles.size() / 3, NBP_GRID_LANES, 0, (const nbp_grid_desc *)d[0], d[1], d[2], c->arena,
                      c->N, c->S, dgrid, dext));
  // straight into the caller's buffers (a staging vector of the grids' size costs more than the kernel: profiles/marginal_grid_kernel.txt)
  HIPCHK(hipMemcpyAsync(out, dgrid, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
  if (extent_out) HIPCHK(hipMemcpyAsync(extent_out, dext, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_evaluate
nbp_status nbp_kde_marginal_grid(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw,
                                 const nbp_grid_desc *desc, double *out, double *extent_out) {
  if (!c || !pts || !bw || !desc || !out) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_check(c, "marginal grid", manifold, {{pts, n_pts, bw}}));
  nbp_grid_desc g = *desc;
  g.slot = 0;
  g.manifold = manifold;
  int64_t pts_n = 0;
  NBPCHK(grid_desc_check(c, g, 0, &pts_n));  // (before slot 0 is touched)
  NBPCHK(kde_write(c, manifold, {{pts, n_pts, bw}}));
  const int32_t first[2] = {0, (int32_t)pts_n};
  return nbp_run_marginal_grid(c, &g, 1, first, out, extent_out);
}

// p_K at query points: nbp_run_evaluate's launch with the masked instance of its kernel
nbp_status nbp_run_evaluate_marginal(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                     const int32_t *q_first, const double *queries, double *dens_out) {
  if (!c || ((!slots || !manifolds || !masks || !q_first) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  if (q_first[0] != 0) return fail(NBP_ERR_ARG, "evaluate marginal: q_first[0] must be 0");
  NBPCHK(batch_check(c, "evaluate marginal", {slots}, manifolds, n, [&](int i) {
    return q_first[i + 1] < q_first[i] ? refusal{NBP_ERR_ARG, "q_first must not decrease"} : mask_refusal(manifolds[i], masks[i]);
  }));
  return run_point_density(c, slots, manifolds, masks, n, q_first, queries, dens_out);
}

// mmd(p1, p2, varType; bw = [sigma]) (services/SolverUtilities.jl:25-47) for pairs of beliefs resident in slots: one workgroup per
// pair (nbp_query.h), one copy back
nbp_status nbp_run_mmd(nbp_ctx *c, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, int32_t n, double sigma,
                       double *mmd_out) {
  if (!c || ((!slots_a || !slots_b || !manifolds || !mmd_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (!(sigma >= 0.0 && sigma < INFINITY)) return fail(NBP_ERR_ARG, "mmd: sigma must be finite and not negative");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "mmd", {slots_a, slots_b}, manifolds, n, no_refusal));
  const int32_t *d[3];
  NBPCHK(stage_columns(c, {{slots_a, 4 * (size_t)n}, {slots_b, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}}, d, (size_t)n));
  NBPCHK(launch_checked(c, nbp_mmd_kernel, n, c->Npad, nbp_mmd_lds_bytes(c->N), d[0], d[1], d[2], c->arena, c->N, c->S, sigma, c->query));
  return query_fetch(c, mmd_out, c->query, sizeof(double) * (size_t)n);
}

// host-buffer form: stages through slots 0 and 1 (which it clobbers).  The bandwidths play no part in an mmd; the slots carry ones.
nbp_status nbp_kde_mmd(nbp_ctx *c, int32_t manifold, const double *a, int32_t na, const double *b, int32_t nb, double sigma,
                       double *mmd_out) {
  if (!c || !a || !b || !mmd_out) return fail(NBP_ERR_ARG, "null argument");
  if (!(sigma >= 0.0 && sigma < INFINITY)) return fail(NBP_ERR_ARG, "mmd: sigma must be finite and not negative");
  NBPCHK(kde_stage(c, "mmd", manifold, {{a, na, nullptr}, {b, nb, nullptr}}));
  const int32_t sa = 0, sb = 1;
  return nbp_run_mmd(c, &sa, &sb, &manifold, 1, sigma, mmd_out);
}

// calcMeanCovar (VariableStatistics.jl:39-44) of resident beliefs: one workgroup per belief (nbp_stats.h), one copy back
nbp_status nbp_run_meancov(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, double *mean_out, double *cov_out) {
  if (!c || ((!slots || !manifolds || !mean_out || !cov_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "meancov", {slots}, manifolds, n, no_refusal));
  static_assert(sizeof(nbp_meancov_rec) == sizeof(double) * (NBP_MAXD + NBP_MAXD * NBP_MAXD), "nbp_meancov_rec is packed doubles");
  std::vector<nbp_meancov_rec> rec((size_t)n);
  const scratch_layout q{{sizeof(nbp_meancov_rec), (size_t)n, rec.data()}};
  const int32_t *d[2];
  NBPCHK(stage_columns(c, {{slots, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_meancov_kernel, n, c->Npad, nbp_meancov_lds_bytes(c->N), d[0], d[1], c->arena, c->N, c->S,
                        (nbp_meancov_rec *)q.at(c, 0)));
  NBPCHK(q.fetch(c));
  for (int i = 0; i < n; i++) {
    memcpy(mean_out + (size_t)i * NBP_MAXD, rec[i].mean, sizeof(rec[i].mean));
    memcpy(cov_out + (size_t)i * NBP_MAXD * NBP_MAXD, rec[i].cov, sizeof(rec[i].cov));
  }
  return NBP_OK;
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_ppe.  The bandwidth plays no part; the slot carries ones.
nbp_status nbp_kde_meancov(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, double *mean_out, double *cov_out) {
  if (!c || !pts || !mean_out || !cov_out) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_stage(c, "meancov", manifold, {{pts, n_pts, nullptr}}));
  const int32_t slot = 0;
  double mean3[NBP_MAXD], cov9[NBP_MAXD * NBP_MAXD];
  NBPCHK(nbp_run_meancov(c, &slot, &manifold, 1, mean3, cov9));
  const int D = manifold_dim_h(manifold);
  for (int k = 0; k < D; k++) {
    mean_out[k] = mean3[k];
    for (int e = 0; e < D; e++) cov_out[k * D + e] = cov9[k * NBP_MAXD + e];
  }
  return NBP_OK;
}

// kld(p, q) (attic/examples/FixedPointIllustrationsSquare.jl:53-62) for pairs of beliefs resident in slots: one workgroup per pair
// (nbp_stats.h), one copy back
nbp_status nbp_run_kld(nbp_ctx *c, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, int32_t n, double *kld_out,
                       double *terms_out) {
  if (!c || ((!slots_a || !slots_b || !manifolds || !kld_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "kld", {slots_a, slots_b}, manifolds, n, no_refusal));
  static_assert(sizeof(nbp_kld_rec) == sizeof(double) * 3, "nbp_kld_rec is packed doubles");
  std::vector<nbp_kld_rec> rec((size_t)n);
  const scratch_layout q{{sizeof(nbp_kld_rec), (size_t)n, rec.data()}};
  const int32_t *d[3];
  NBPCHK(stage_columns(c, {{slots_a, 4 * (size_t)n}, {slots_b, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_kld_kernel, n, c->Npad, nbp_kld_lds_bytes(c->N), d[0], d[1], d[2], c->arena, c->N, c->S, (nbp_kld_rec *)q.at(c, 0)));
  NBPCHK(q.fetch(c));
  for (int i = 0; i < n; i++) {
    kld_out[i] = rec[i].kld;
    if (terms_out) {
      terms_out[2 * (size_t)i] = rec[i].eaa;
      terms_out[2 * (size_t)i + 1] = rec[i].eab;
    }
  }
  return NBP_OK;
}

// host-buffer form: stages through slots 0 and 1 (which it clobbers)
nbp_status nbp_kde_kld(nbp_ctx *c, int32_t manifold, const double *a, int32_t na, const double *bw_a, const double *b, int32_t nb,
                       const double *bw_b, double *kld_out, double *terms_out) {
  if (!c || !a || !bw_a || !b || !bw_b || !kld_out) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_stage(c, "kld", manifold, {{a, na, bw_a}, {b, nb, bw_b}}));
  const int32_t sa = 0, sb = 1;
  return nbp_run_kld(c, &sa, &sb, &manifold, 1, kld_out, terms_out);
}

// ---- belief overlaps (nbp_overlap.h) ---------------------------------------------------------------------------------------------
// the kinds of a mask's coordinates (mask_refusal has let it pass) in ascending order: one bit each (1: circular), behind the length << 4
static int overlap_kinds(int32_t manifold, int32_t mask) {
  int kinds = 0, len = 0;
  for (int d = 0; d < manifold_dim_h(manifold); d++)
    if (mask >> d & 1) {
      if (manifold_circ_h(manifold, d)) kinds |= 1 << len;
      len++;
    }
  return kinds | len << 4;
}
// what both forms of the pair entry refuse, pair by pair
static nbp_status overlap_check(nbp_ctx *c, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds_a,
                                const int32_t *manifolds_b, const int32_t *masks_a, const int32_t *masks_b, int32_t n) {
  return batch_check(c, "overlap", {slots_a, slots_b}, manifolds_a, n, [&](int i) {
    if (!manifold_ok(manifolds_b[i])) return refusal{NBP_ERR_ARG, "unknown manifold"};
    for (const refusal &r : {mask_refusal(manifolds_a[i], masks_a[i]), mask_refusal(manifolds_b[i], masks_b[i])})
      if (r.what) return r;
    if (overlap_kinds(manifolds_a[i], masks_a[i]) != overlap_kinds(manifolds_b[i], masks_b[i]))
      return refusal{NBP_ERR_ARG, "inadmissible pair: the masked coordinates differ in number or kind"};
    return refusal{NBP_OK, nullptr};
  });
}

// the overlap coefficient of pairs of beliefs resident in slots: one workgroup per pair (nbp_overlap.h), one copy back
nbp_status nbp_run_overlap(nbp_ctx *c, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds_a, const int32_t *manifolds_b,
                           const int32_t *masks_a, const int32_t *masks_b, int32_t n, nbp_overlap_rec *recs_out) {
  if (!c || ((!slots_a || !slots_b || !manifolds_a || !manifolds_b || !masks_a || !masks_b || !recs_out) && n > 0))
    return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(overlap_check(c, slots_a, slots_b, manifolds_a, manifolds_b, masks_a, masks_b, n));
  static_assert(sizeof(nbp_overlap_rec) == sizeof(double) * 4, "nbp_overlap_rec is packed doubles");
  const int32_t *d[6];
  const size_t col = 4 * (size_t)n;
  NBPCHK(stage_columns(c, {{slots_a, col}, {slots_b, col}, {manifolds_a, col}, {manifolds_b, col}, {masks_a, col}, {masks_b, col}}, d,
                       (size_t)n * 4));
  NBPCHK(launch_checked(c, nbp_overlap_kernel, n, c->Npad, nbp_overlap_lds_bytes(c->N), d[0], d[1], d[2], d[3], d[4], d[5], c->arena, c->N,
                        c->S, (nbp_overlap_rec *)c->query));
  return query_fetch(c, recs_out, c->query, sizeof(nbp_overlap_rec) * (size_t)n);
}

// host-buffer form: stages through slots 0 and 1 (which it clobbers)
nbp_status nbp_kde_overlap(nbp_ctx *c, int32_t manifold_a, const double *a, int32_t na, const double *bw_a, int32_t mask_a,
                           int32_t manifold_b, const double *b, int32_t nb, const double *bw_b, int32_t mask_b, nbp_overlap_rec *rec_out) {
  if (!c || !a || !bw_a || !b || !bw_b || !rec_out) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_check(c, "overlap", manifold_a, {{a, na, bw_a}, {b, nb, bw_b}}));
  if (!manifold_ok(manifold_b)) return fail(NBP_ERR_ARG, "overlap: unknown manifold");  // (kde_check's wording, for the second belief)
  const int32_t sa = 0, sb = 1;
  NBPCHK(overlap_check(c, &sa, &sb, &manifold_a, &manifold_b, &mask_a, &mask_b, 1));
  NBPCHK(nbp_belief_write(c, 0, manifold_a, a, na, bw_a, nullptr));
  NBPCHK(nbp_belief_write(c, 1, manifold_b, b, nb, bw_b, nullptr));
  return nbp_run_overlap(c, &sa, &sb, &manifold_a, &manifold_b, &mask_a, &mask_b, 1, rec_out);
}

// the options as given, or the defaults; refused before anything is launched
static nbp_status overlap_opts_check(const nbp_ctx *c, const nbp_overlap_opts *opts, nbp_overlap_opts *o) {
  *o = opts ? *opts : nbp_overlap_opts{NBP_OVERLAP_REACH, NBP_OVERLAP_MIN_COEFF, NBP_OVERLAP_TOPK, 0};
  o->pad = 0;
  if (!(o->reach > 0.0 && o->reach < INFINITY)) return fail(NBP_ERR_ARG, "overlap search: reach must be positive and finite");
  if (!(o->min_coeff > 0.0 && o->min_coeff < INFINITY)) return fail(NBP_ERR_ARG, "overlap search: min_coeff must be positive and finite");
  if (o->topk < 1 || o->topk > NBP_OVERLAP_MAXK) return fail(NBP_ERR_RANGE, "overlap search: topk outside 1 .. " + std::to_string(NBP_OVERLAP_MAXK));
  // a skipped pair has logc <= log(N) - reach^2 / 2; one nat on top swallows every rounding
  if (!(std::log(o->min_coeff) >= std::log((double)c->N) - 0.5 * (o->reach * o->reach) + 1.0))
    return fail(NBP_ERR_RANGE, "overlap search: log(min_coeff) must be at least log(N) - reach^2 / 2 + 1 (a skipped pair could pass the threshold)");
  return NBP_OK;
}

// the search over a list of beliefs resident in slots: the per-belief preparation, then one workgroup per row (nbp_overlap.h); one
// copy back
nbp_status nbp_run_overlap_search(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                  const nbp_overlap_opts *opts, int32_t *idx_out, double *logc_out, int32_t *found_out,
                                  int32_t *evaluated_out) {
  if (!c || ((!slots || !manifolds || !masks || !idx_out || !logc_out || !found_out || !evaluated_out) && n > 0))
    return fail(NBP_ERR_ARG, "null argument");
  nbp_overlap_opts o;
  NBPCHK(overlap_opts_check(c, opts, &o));
  if (n <= 0) return NBP_OK;
  int first = 0;
  NBPCHK(batch_check(c, "overlap search", {slots}, manifolds, n, [&](int i) {
    const refusal r = mask_refusal(manifolds[i], masks[i]);
    if (r.what) return r;
    const int k = overlap_kinds(manifolds[i], masks[i]);
    if (i == 0) first = k;
    return k != first ? refusal{NBP_ERR_ARG, "not admissible against belief 0: the masked coordinates differ in number or kind"} : r;
  }));
  // the query scratch: prep[n] | logc[n topk] | idx[n topk] | found[n] | evaluated[n] (the last three int32): one copy back from logc on
  static_assert(sizeof(nbp_overlap_prep) % sizeof(double) == 0, "nbp_overlap_prep fills whole doubles of the query scratch");
  const size_t V = (size_t)n, K = (size_t)o.topk;
  const scratch_layout q{{sizeof(nbp_overlap_prep), V, nullptr}, {sizeof(double), V * K, logc_out}, {4, V * K, idx_out}, {4, V, found_out},
                         {4, V, evaluated_out}};
  const int32_t *d[3];
  NBPCHK(stage_columns(c, {{slots, 4 * V}, {manifolds, 4 * V}, {masks, 4 * V}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_overlap_prep_kernel, V, c->Npad, nbp_overlap_prep_lds_bytes(c->N), d[0], d[1], d[2], c->arena, c->N, c->S,
                        (nbp_overlap_prep *)q.at(c, 0)));
  NBPCHK(launch_checked(c, nbp_overlap_search_kernel, V, c->Npad, nbp_overlap_search_lds_bytes(c->N), d[0], d[1], d[2], n, c->arena, c->N,
                        c->S, (const nbp_overlap_prep *)q.at(c, 0), o.reach * o.reach, std::log(o.min_coeff), o.topk, (int32_t *)q.at(c, 2),
                        q.at(c, 1), (int32_t *)q.at(c, 3), (int32_t *)q.at(c, 4)));
  return q.fetch(c);
}

// ---- scene densities (nbp_scene.h) -------------------------------------------------------------------------------------------------
// what the scene entry refuses in its descriptor, whatever the list holds
static nbp_status scene_desc_check(const nbp_scene_desc &g) {
  const std::string who = "scene grid: ";
  if (g.flags & ~NBP_SCENE_AUTO_EXTENT) return fail(NBP_ERR_ARG, who + "unknown flag");
  if (!std::isfinite(g.margin)) return fail(NBP_ERR_ARG, who + "margin not finite");
  if (!(g.reach > 0.0)) return fail(NBP_ERR_ARG, who + "reach must be positive (+inf: no culling)");
  for (int a = 0; a < 2; a++)
    if (g.n[a] < 1 || g.n[a] > NBP_SCENE_MAX) return fail(NBP_ERR_RANGE, who + "n outside 1 .. " + std::to_string(NBP_SCENE_MAX));
  if ((int64_t)g.n[0] * g.n[1] > ((int64_t)1 << 22)) return fail(NBP_ERR_RANGE, who + "more than 2^22 grid points");
  return NBP_OK;
}

// Every belief of a list of resident beliefs on one grid: the per-belief preparation, the extent where it is automatic, one wave per
// tile (nbp_scene.h).  The columns (and an explicit extent) go up in one staging copy; the number of tiles depends on n alone, so
// nothing comes back between the launches; the grid (and the owners) are copied straight into the caller's buffers, whatever else
// was asked for in one more copy (scratch_layout::fetch_split).
nbp_status nbp_run_scene_grid(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *dims, const double *weights,
                              int32_t V, const nbp_scene_desc *desc, double *out, int32_t *owner_out, int32_t *skipped_out,
                              double *extent_out, int64_t *tile_beliefs_out) {
  if (!c || !desc || !out || V < 0 || ((!slots || !manifolds || !dims) && V > 0)) return fail(NBP_ERR_ARG, "scene grid: null argument or V < 0");
  const nbp_scene_desc g = *desc;
  NBPCHK(scene_desc_check(g));
  const bool autoext = g.flags & NBP_SCENE_AUTO_EXTENT;
  const size_t pts = (size_t)g.n[0] * (size_t)g.n[1];
  const int axes = V > 0 && dims[1] == -1 ? 1 : 2;  // (belief 0 sets the shape of the scene)
  int circ = 0;
  NBPCHK(batch_check(c, "scene grid", {slots}, manifolds, V, [&](int i) {
    const int D = manifold_dim_h(manifolds[i]), d0 = dims[2 * i], d1 = dims[2 * i + 1];
    if (d0 < 0 || d0 >= D || d1 < -1 || d1 >= D) return refusal{NBP_ERR_RANGE, "coordinate outside the manifold"};
    if (d1 == d0) return refusal{NBP_ERR_RANGE, "repeated coordinate"};
    int kinds = manifold_circ_h(manifolds[i], d0) ? 1 : 0;
    if (d1 >= 0 && manifold_circ_h(manifolds[i], d1)) kinds |= 2;
    if (i == 0) circ = kinds;
    if ((d1 == -1 ? 1 : 2) != axes || kinds != circ)
      return refusal{NBP_ERR_ARG, "not admissible against belief 0: the coordinates differ in number or kind"};
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) return refusal{NBP_ERR_ARG, "weight negative or not finite"};
    return refusal{NBP_OK, nullptr};
  }));
  if (V > 0 && axes == 1 && g.n[1] != 1) return fail(NBP_ERR_RANGE, "scene grid: a 1-D scene has n[1] = 1");
  for (int a = 0; a < axes; a++) {
    if (autoext && V > 0 && !(circ >> a & 1) && g.n[a] < 2) return fail(NBP_ERR_RANGE, "scene grid: automatic extent of a Euclidean axis needs n >= 2");
    if (!autoext && !std::isfinite(g.lo[a])) return fail(NBP_ERR_RANGE, "scene grid: lo not finite");
    if (!autoext && !(g.step[a] > 0.0 && std::isfinite(g.step[a]))) return fail(NBP_ERR_RANGE, "scene grid: step must be finite and positive");
  }
  double ext[4] = {0.0, 0.0, 0.0, 0.0};
  if (!autoext)
    for (int a = 0; a < axes; a++) ext[2 * a] = g.lo[a], ext[2 * a + 1] = g.step[a];
  if (V == 0) {  // nothing to add: a grid of zeros, nobody's
    std::fill(out, out + pts, 0.0);
    if (owner_out) std::fill(owner_out, owner_out + pts, -1);
    if (extent_out) memcpy(extent_out, ext, sizeof(ext));
    if (tile_beliefs_out) *tile_beliefs_out = 0;
    return NBP_OK;
  }
  const bool two = axes == 2;
  const size_t tiles = two ? (size_t)((g.n[0] + NBP_GRID_TILE - 1) / NBP_GRID_TILE) * (size_t)((g.n[1] + NBP_GRID_TILE - 1) / NBP_GRID_TILE)
                           : (size_t)((g.n[0] + NBP_GRID_TILE1 - 1) / NBP_GRID_TILE1);
  std::vector<int32_t> counts(tile_beliefs_out ? tiles : 0);
  // the query scratch: records | skipped | extent | tile counts | grid | owners; the small parts come back in one copy
  static_assert(sizeof(nbp_scene_rec) % sizeof(double) == 0, "nbp_scene_rec fills whole doubles of the query scratch");
  const size_t n = (size_t)V;
  const scratch_layout q{{sizeof(nbp_scene_rec), n, nullptr}, {4, n, skipped_out}, {sizeof(double), 4, autoext ? extent_out : nullptr},
                         {4, tiles, tile_beliefs_out ? counts.data() : nullptr}, {sizeof(double), pts, out}, {4, owner_out ? pts : 0, owner_out}};
  const int32_t *d[5];
  NBPCHK(stage_columns(c, {{slots, 4 * n}, {manifolds, 4 * n}, {dims, 8 * n}, {weights, weights ? 8 * n : 0}, {ext, sizeof(ext)}}, d, q.total()));
  nbp_scene_rec *recs = (nbp_scene_rec *)q.at(c, 0);
  const double *dw = weights ? (const double *)d[3] : nullptr, *dext = autoext ? q.at(c, 2) : (const double *)d[4];
  NBPCHK(launch_checked(c, nbp_scene_prep_kernel, n, c->Npad, 0, d[0], d[1], d[2], (const double *)c->arena, c->N, c->S, g.margin, g.reach, recs,
                        (int32_t *)q.at(c, 1)));
  if (autoext)
    NBPCHK(launch_checked(c, nbp_scene_extent_kernel, 1, NBP_GRID_LANES, 0, (const nbp_scene_rec *)recs, (int)V, (int)two, circ, (int)g.n[0],
                          (int)g.n[1], q.at(c, 2)));
  NBPCHK(launch_checked(c, owner_out ? nbp_scene_grid_owner_kernel : nbp_scene_grid_kernel, tiles, NBP_GRID_LANES, 0, (const nbp_scene_rec *)recs,
                        d[0], d[2], dw, (int)V, (const double *)c->arena, c->N, c->S, (int)two, circ, (int)g.n[0], (int)g.n[1], dext, q.at(c, 4),
                        (int32_t *)q.at(c, 5), (int32_t *)q.at(c, 3)));
  NBPCHK(q.fetch_split(c, 4));  // (the grid and the owners straight into the caller's buffers)
  if (extent_out && !autoext) memcpy(extent_out, ext, sizeof(ext));
  if (tile_beliefs_out) {
    int64_t sum = 0;
    for (int32_t k : counts) sum += k;
    *tile_beliefs_out = sum;
  }
  return NBP_OK;
}

// ---- credible regions (nbp_credible.h) -------------------------------------------------------------------------------------------
// the options of a credible-region batch; refused before anything is launched, naming the entry
static nbp_status credible_opts_check(const nbp_credible_opts *o) {
  const std::string lim = std::to_string(NBP_CRED_MAX);
  if (o->n_mass < 0 || o->n_mass > NBP_CRED_MAX) return fail(NBP_ERR_RANGE, "credible: n_mass outside 0 .. " + lim);
  if (o->n_prob < 0 || o->n_prob > NBP_CRED_MAX) return fail(NBP_ERR_RANGE, "credible: n_prob outside 0 .. " + lim);
  for (int a = 0; a < o->n_mass; a++)  // (a NaN fails both comparisons)
    if (!(o->mass[a] > 0.0 && o->mass[a] <= 1.0)) return fail(NBP_ERR_RANGE, "credible: mass " + std::to_string(a) + " outside (0, 1]");
  for (int p = 0; p < o->n_prob; p++)
    if (!(o->prob[p] >= 0.0 && o->prob[p] <= 1.0)) return fail(NBP_ERR_RANGE, "credible: probability " + std::to_string(p) + " outside [0, 1]");
  return NBP_OK;
}

// what both forms of the credible entry refuse: the options, then belief by belief the mask and the queries
static nbp_status credible_check(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                 const nbp_credible_opts *opts, const int32_t *q_first, const double *queries,
                                 const nbp_credibility_rec *qrec_out) {
  NBPCHK(credible_opts_check(opts));
  if (q_first && q_first[0] != 0) return fail(NBP_ERR_RANGE, "credible: belief 0: q_first must ascend from 0");
  return batch_check(c, "credible", {slots}, manifolds, n, [&](int i) {
    const refusal r = mask_refusal(manifolds[i], masks[i]);
    if (r.what || !q_first) return r;
    if (q_first[i + 1] < q_first[i]) return refusal{NBP_ERR_RANGE, "q_first must ascend from 0"};
    if (q_first[i + 1] > q_first[i] && (!queries || !qrec_out)) return refusal{NBP_ERR_ARG, "null argument"};
    for (int32_t q = q_first[i]; q < q_first[i + 1]; q++)
      for (int d = 0; d < NBP_MAXD; d++)
        if ((masks[i] >> d & 1) && !std::isfinite(queries[(size_t)q * NBP_MAXD + d]))
          return refusal{NBP_ERR_RANGE, "a query entry is not finite"};
    return refusal{NBP_OK, nullptr};
  });
}

// HDR levels, credibility of reference points and coordinate quantiles of beliefs resident in slots: one workgroup per belief
// (nbp_credible.h).  Columns, options and queries go up in one staging copy; records, query records and the optional per-particle
// outputs come back in one copy.
nbp_status nbp_run_credible(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                            const nbp_credible_opts *opts, const int32_t *q_first, const double *queries, nbp_credible_rec *rec_out,
                            double *logdens_out, int32_t *order_out, nbp_credibility_rec *qrec_out) {
  if (!c || ((!slots || !manifolds || !masks || !opts || !rec_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(credible_check(c, slots, manifolds, masks, n, opts, q_first, queries, qrec_out));
  static_assert(sizeof(nbp_credible_rec) % sizeof(double) == 0 && sizeof(nbp_credibility_rec) % sizeof(double) == 0,
                "the credible records fill whole doubles of the query scratch");
  static_assert(sizeof(nbp_credible_opts) % sizeof(double) == 0, "nbp_credible_opts fills whole doubles of the staging copy");
  const size_t V = (size_t)n, Q = q_first ? (size_t)q_first[n] : 0, N = (size_t)c->N;
  // the query scratch: rec[n] | qrec[Q] | logdens[n N] | order[n N] (int32); the last two only where the caller asks for them
  const scratch_layout q{{sizeof(nbp_credible_rec), V, rec_out}, {sizeof(nbp_credibility_rec), Q, qrec_out},
                         {sizeof(double), logdens_out ? V * N : 0, logdens_out}, {4, order_out ? V * N : 0, order_out}};
  const int32_t *d[6];
  NBPCHK(stage_columns(c, {{slots, 4 * V}, {manifolds, 4 * V}, {masks, 4 * V}, {opts, sizeof(nbp_credible_opts)},
                           {q_first, q_first ? 4 * (V + 1) : 0}, {queries, sizeof(double) * NBP_MAXD * Q}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_credible_kernel, V, c->Npad, nbp_credible_lds_bytes(c->N), d[0], d[1], d[2], (const nbp_credible_opts *)d[3],
                        q_first ? d[4] : (const int32_t *)nullptr, (const double *)d[5], c->arena, c->N, c->S, (nbp_credible_rec *)q.at(c, 0),
                        logdens_out ? q.at(c, 2) : (double *)nullptr, order_out ? (int32_t *)q.at(c, 3) : (int32_t *)nullptr,
                        (nbp_credibility_rec *)q.at(c, 1)));
  return q.fetch(c);
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_meancov; everything is checked before slot 0 is touched
nbp_status nbp_kde_credible(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, int32_t mask,
                            const nbp_credible_opts *opts, const double *queries, int32_t nq, nbp_credible_rec *rec_out,
                            double *logdens_out, int32_t *order_out, nbp_credibility_rec *qrec_out) {
  if (!c || !pts || !bw || !opts || !rec_out || ((!queries || !qrec_out) && nq > 0)) return fail(NBP_ERR_ARG, "null argument");
  NBPCHK(kde_check(c, "credible", manifold, {{pts, n_pts, bw}}));
  if (nq < 0) return fail(NBP_ERR_ARG, "credible: nq < 0");
  const int32_t slot = 0, q_first[2] = {0, nq};
  NBPCHK(credible_check(c, &slot, &manifold, &mask, 1, opts, q_first, queries, qrec_out));
  // (a bandwidth entry outside the mask is not read by the kernel, but the slot write wants a full vector: the caller's is passed on)
  NBPCHK(kde_write(c, manifold, {{pts, n_pts, bw}}));
  return nbp_run_credible(c, &slot, &manifold, &mask, 1, opts, q_first, queries, rec_out, logdens_out, order_out, qrec_out);
}

// ---- modes of beliefs (nbp_modes.h) ----------------------------------------------------------------------------------------------
// the options as given, or the defaults; refused before anything is launched
static nbp_status modes_opts_check(const nbp_modes_opts *opts, nbp_modes_opts *o) {
  *o = opts ? *opts : nbp_modes_opts{NBP_MODES_BW_SCALE, NBP_MODES_TOL, NBP_MODES_MERGE, NBP_MODES_MAX_ITER, 0};
  o->pad = 0;
  if (!(o->bw_scale > 0.0 && o->bw_scale < INFINITY)) return fail(NBP_ERR_ARG, "modes: bw_scale must be positive and finite");
  if (!(o->tol > 0.0 && o->tol < INFINITY)) return fail(NBP_ERR_ARG, "modes: tol must be positive and finite");
  if (!(o->merge > 0.0 && o->merge < INFINITY)) return fail(NBP_ERR_ARG, "modes: merge must be positive and finite");
  if (o->max_iter < 1) return fail(NBP_ERR_ARG, "modes: max_iter must be at least 1");
  if (o->merge < 1000.0 * o->tol) return fail(NBP_ERR_RANGE, "modes: merge must be at least 1000 tol");
  return NBP_OK;
}

// mean-shift modes of resident beliefs: one workgroup per belief (nbp_modes.h), one copy back.  The query scratch holds
// hdr[n][2] | recs[n][NBP_MODES_MAX] | labels[n][N] | iters[n][N], each part starting on a whole double; the copy ends behind the last part asked for
nbp_status nbp_run_modes(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, const nbp_modes_opts *opts,
                         nbp_mode_rec *recs_out, int32_t *n_modes_out, int32_t *labels_out, int32_t *iters_out, int32_t *n_unconverged_out) {
  if (!c || ((!slots || !manifolds || !recs_out || !n_modes_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  nbp_modes_opts o;
  NBPCHK(modes_opts_check(opts, &o));
  NBPCHK(batch_check(c, "modes", {slots}, manifolds, n, no_refusal));
  static_assert(sizeof(nbp_mode_rec) % sizeof(double) == 0, "nbp_mode_rec fills whole doubles of the query scratch");
  const size_t V = (size_t)n, rows = V * (size_t)c->N;
  std::vector<int32_t> hh(2 * V);
  const scratch_layout q{{4, 2 * V, hh.data()}, {sizeof(nbp_mode_rec), V * NBP_MODES_MAX, recs_out}, {4, rows, labels_out}, {4, rows, iters_out}};
  const int32_t *d[2];
  NBPCHK(stage_columns(c, {{slots, 4 * V}, {manifolds, 4 * V}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_modes_kernel, n, c->Npad, nbp_modes_lds_bytes(c->N), d[0], d[1], c->arena, c->N, c->S, o,
                        (nbp_mode_rec *)q.at(c, 1), (int32_t *)q.at(c, 0), (int32_t *)q.at(c, 2), (int32_t *)q.at(c, 3)));
  NBPCHK(q.fetch(c));
  for (int i = 0; i < n; i++) {
    n_modes_out[i] = hh[2 * i];
    if (n_unconverged_out) n_unconverged_out[i] = hh[2 * i + 1];
  }
  return NBP_OK;
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_ppe.  A belief of more than N points keeps its first N
// (nbp_belief_write): the rows of labels_out / iters_out beyond them are -1 / 0.
nbp_status nbp_kde_modes(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, const nbp_modes_opts *opts,
                         nbp_mode_rec *recs_out, int32_t *n_modes_out, int32_t *labels_out, int32_t *iters_out, int32_t *n_unconverged_out) {
  if (!c || !pts || !bw || !recs_out || !n_modes_out) return fail(NBP_ERR_ARG, "null argument");
  nbp_modes_opts o;
  NBPCHK(modes_opts_check(opts, &o));
  NBPCHK(kde_stage(c, "modes", manifold, {{pts, n_pts, bw}}));
  const int32_t slot = 0;
  std::vector<int32_t> lab(labels_out ? (size_t)c->N : 0), its(iters_out ? (size_t)c->N : 0);
  NBPCHK(nbp_run_modes(c, &slot, &manifold, 1, &o, recs_out, n_modes_out, labels_out ? lab.data() : nullptr, iters_out ? its.data() : nullptr,
                       n_unconverged_out));
  for (int i = 0; i < n_pts; i++) {
    if (labels_out) labels_out[i] = i < c->N ? lab[i] : -1;
    if (iters_out) iters_out[i] = i < c->N ? its[i] : 0;
  }
  return NBP_OK;
}

// ---- mixture summaries of beliefs (nbp_mixture.h) ----------------------------------------------------------------------------------
// the options as given, or the defaults; refused before anything is launched
static nbp_status mixture_opts_check(const nbp_mixture_opts *opts, nbp_mixture_opts *o) {
  *o = opts ? *opts : nbp_mixture_opts{NBP_MIX_TOL, NBP_MIX_MAX_ITER, 0};
  o->pad = 0;
  if (!(o->tol >= 0.0 && o->tol < INFINITY)) return fail(NBP_ERR_ARG, "mixture: tol must be finite and not negative");
  if (o->max_iter < 1) return fail(NBP_ERR_ARG, "mixture: max_iter must be at least 1");
  return NBP_OK;
}
static nbp_status mixture_labels_check(const int32_t *lab, size_t cnt, int belief) {
  for (size_t k = 0; k < cnt; k++)
    if (lab[k] < -1 || lab[k] >= NBP_MIX_MAX)
      return fail(NBP_ERR_ARG, "mixture: belief " + std::to_string(belief) + ": label " + std::to_string(k) + " outside -1 .. NBP_MIX_MAX - 1");
  return NBP_OK;
}

// Gaussian-mixture summaries of beliefs resident in slots: one workgroup per belief runs the whole EM (nbp_mixture.h).  The label
// rows the items name are gathered on the host (a row no item names is not read), so the columns, the rows and the starting means
// go up in one staging copy; the records and the optional labels come back in one copy.
nbp_status nbp_run_mixture(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, const int32_t *labels, const int32_t *row,
                           const double *init_mean, const nbp_mixture_opts *opts, nbp_mixture_rec *recs_out, int32_t *labels_out) {
  if (!c || ((!slots || !manifolds || !labels || !row || !init_mean || !recs_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  nbp_mixture_opts o;
  NBPCHK(mixture_opts_check(opts, &o));
  NBPCHK(batch_check(c, "mixture", {slots}, manifolds, n, [&](int i) {
    return row[i] < 0 ? refusal{NBP_ERR_ARG, "a negative label row"} : refusal{NBP_OK, nullptr};
  }));
  const size_t V = (size_t)n, N = (size_t)c->N;
  std::vector<int32_t> rows(V * N);
  for (size_t i = 0; i < V; i++) {
    NBPCHK(mixture_labels_check(labels + (size_t)row[i] * N, N, (int)i));
    memcpy(rows.data() + i * N, labels + (size_t)row[i] * N, 4 * N);
  }
  static_assert(sizeof(nbp_mixture_rec) % sizeof(double) == 0, "nbp_mixture_rec fills whole doubles of the query scratch");
  const scratch_layout q{{sizeof(nbp_mixture_rec), V, recs_out}, {4, labels_out ? V * N : 0, labels_out}};
  const int32_t *d[4];
  NBPCHK(stage_columns(c, {{slots, 4 * V}, {manifolds, 4 * V}, {rows.data(), 4 * V * N}, {init_mean, sizeof(double) * NBP_MIX_MAX * NBP_MAXD * V}},
                       d, q.total()));
  NBPCHK(launch_checked(c, nbp_mixture_kernel, V, c->Npad, nbp_mixture_lds_bytes(c->N), d[0], d[1], d[2], (const double *)d[3], c->arena, c->N,
                        c->S, o, (nbp_mixture_rec *)q.at(c, 0), labels_out ? (int32_t *)q.at(c, 1) : (int32_t *)nullptr));
  return q.fetch(c);
}

// host-buffer form: stages through slot 0 (which it clobbers), like nbp_kde_modes; everything is checked before slot 0 is touched.
// The label row is padded with -1.
nbp_status nbp_kde_mixture(nbp_ctx *c, int32_t manifold, const double *pts, int32_t n_pts, const double *bw, const int32_t *labels,
                           const double *init_mean, const nbp_mixture_opts *opts, nbp_mixture_rec *rec_out, int32_t *labels_out) {
  if (!c || !pts || !bw || !labels || !init_mean || !rec_out) return fail(NBP_ERR_ARG, "null argument");
  nbp_mixture_opts o;
  NBPCHK(mixture_opts_check(opts, &o));
  NBPCHK(kde_check(c, "mixture", manifold, {{pts, n_pts, bw}}));
  const int N = c->N, kept = n_pts < N ? n_pts : N;
  NBPCHK(mixture_labels_check(labels, (size_t)kept, 0));
  NBPCHK(kde_write(c, manifold, {{pts, n_pts, bw}}));
  std::vector<int32_t> lab((size_t)N, -1), out(labels_out ? (size_t)N : 0);
  memcpy(lab.data(), labels, 4 * (size_t)kept);
  const int32_t slot = 0, row = 0;
  NBPCHK(nbp_run_mixture(c, &slot, &manifold, 1, lab.data(), &row, init_mean, &o, rec_out, labels_out ? out.data() : nullptr));
  if (labels_out)
    for (int i = 0; i < n_pts; i++) labels_out[i] = i < N ? out[i] : -1;
  return NBP_OK;
}

// ---- factor likelihoods (nbp_likelihood.h) -----------------------------------------------------------------------------------------
// what nbp_run_factor_likelihood refuses in one descriptor (the slots apart)
static refusal likelihood_refusal(const nbp_likelihood_desc &p) {
  const auto posfin = [](double v) { return v > 0.0 && v < INFINITY; };
  if (p.kind == NBP_F_MSGPRIOR || p.kind == NBP_F_PASSTHROUGH) return {NBP_ERR_ARG, "message priors and pass-through priors have no density in closed form"};
  if (p.kind < NBP_F_PRIOR || p.kind > NBP_F_EUCLIDDIST) return {NBP_ERR_ARG, "unknown factor kind"};
  if (p.kind == NBP_F_CIRCULAR && p.manifold != NBP_CIRCULAR) return {NBP_ERR_ARG, "CircularCircular needs Circular variables"};
  if (p.kind == NBP_F_SE2 && p.manifold != NBP_SE2) return {NBP_ERR_ARG, "SE2 factor needs SE2 variables"};
  if ((p.kind == NBP_F_LINREL || p.kind == NBP_F_EUCLIDDIST) && p.manifold > NBP_EUCLID3)
    return {NBP_ERR_ARG, "LinearRelative and EuclidDistance need Euclid variables"};
  if (p.kind == NBP_F_PRIOR && p.slot_b != -1) return {NBP_ERR_ARG, "a prior is unary: slot_b must be -1"};
  if (p.ncomp < 1 || p.ncomp > NBP_MAXC) return {NBP_ERR_ARG, "ncomp outside 1 .. NBP_MAXC"};
  const int D = manifold_dim_h(p.manifold);
  int zd = (p.kind == NBP_F_CIRCULAR || p.kind == NBP_F_EUCLIDDIST) ? 1 : D;
  if (p.partial_mask) {
    if (p.partial_mask < 0 || p.partial_mask >= (1 << D)) return {NBP_ERR_RANGE, "partial_mask outside the manifold's coordinates"};
    zd = __builtin_popcount(p.partial_mask);
    if (p.kind == NBP_F_LINREL) {
      if (zd > 2) return {NBP_ERR_ARG, "partial LinearRelative: one or two partial coordinates"};
    } else if (p.kind != NBP_F_PRIOR && p.kind != NBP_F_SE2)
      return {NBP_ERR_ARG, "partial_mask is supported for Prior, LinearRelative and SE(2) ManifoldFactor factors"};
  }
  double wsum = 0.0;
  for (int c = 0; c < p.ncomp; c++) {
    const double *q = p.comp[c];
    if (!(q[0] >= 0.0 && q[0] < INFINITY)) return {NBP_ERR_ARG, "a component weight is negative or not finite"};
    wsum += q[0];
    const double fam = zd == 1 ? q[12] : 0.0;
    if (fam == (double)NBP_DIST_TABLE) return {NBP_ERR_ARG, "an alias table has no density"};
    if (fam != (double)NBP_DIST_GAUSSIAN && fam != (double)NBP_DIST_UNIFORM && fam != (double)NBP_DIST_RAYLEIGH)
      return {NBP_ERR_ARG, "unknown measurement family"};
    if (fam == (double)NBP_DIST_UNIFORM) {
      if (!posfin(q[4])) return {NBP_ERR_ARG, "the width of a Uniform is not positive and finite"};
    } else if (fam == (double)NBP_DIST_RAYLEIGH) {
      if (!posfin(q[4])) return {NBP_ERR_ARG, "the sigma of a Rayleigh is not positive and finite"};
    } else {
      for (int i = 0; i < zd; i++) {
        if (!posfin(q[4 + 3 * i + i])) return {NBP_ERR_ARG, "a diagonal entry of L is not positive and finite"};
        for (int j = i + 1; j < zd; j++)
          if (q[4 + 3 * i + j] != 0.0) return {NBP_ERR_ARG, "L has a non-zero above the diagonal"};
      }
    }
  }
  if (!(wsum > 0.0 && wsum < INFINITY)) return {NBP_ERR_ARG, "the component weights have no positive sum"};
  return {NBP_OK, nullptr};
}

// one item, in nbp_run_ppe's order: the slots, the manifold, then the rest of the descriptor (the product grids check their items
// through it as well)
static refusal likelihood_item_refusal(const nbp_ctx *c, const nbp_likelihood_desc &p) {
  refusal r{NBP_OK, nullptr};
  if (p.slot_a < 0 || p.slot_a >= c->n_slots) r = {NBP_ERR_RANGE, "slot_a out of range"};
  else if (p.slot_b != -1 && (p.slot_b < 0 || p.slot_b >= c->n_slots)) r = {NBP_ERR_RANGE, "slot_b out of range"};
  else if (!manifold_ok(p.manifold)) r = {NBP_ERR_ARG, "unknown manifold"};
  else r = likelihood_refusal(p);
  if (!r.what && p.kind != NBP_F_PRIOR && p.slot_b == -1) r = {NBP_ERR_RANGE, "slot_b out of range (a relative factor has two roles)"};
  return r;
}
static nbp_status likelihood_check(nbp_ctx *c, const nbp_likelihood_desc *descs, int n) {
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n; i++) {
    const refusal r = likelihood_item_refusal(c, descs[i]);
    if (r.what) return fail(r.code, "factor_likelihood: item " + std::to_string(i) + ": " + r.what);
  }
  return NBP_OK;
}

// one workgroup per item (nbp_likelihood.h), one upload of the descriptors, one copy back
nbp_status nbp_run_factor_likelihood(nbp_ctx *c, const nbp_likelihood_desc *descs, int32_t n, double *loglik_out, double *comp_loglik_out) {
  if (!c || ((!descs || !loglik_out) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(likelihood_check(c, descs, n));
  static_assert(sizeof(nbp_likelihood_rec) == sizeof(double) * (1 + NBP_MAXC), "nbp_likelihood_rec is packed doubles");
  static_assert(sizeof(nbp_likelihood_desc) % 8 == 0, "nbp_likelihood_desc keeps its doubles aligned in an array");
  std::vector<nbp_likelihood_rec> rec((size_t)n);
  const scratch_layout q{{sizeof(nbp_likelihood_rec), (size_t)n, rec.data()}};
  const int32_t *d[1];
  NBPCHK(stage_columns(c, {{descs, sizeof(nbp_likelihood_desc) * (size_t)n}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_likelihood_kernel, n, c->Npad, nbp_likelihood_lds_bytes(c->N), (const nbp_likelihood_desc *)d[0], c->arena,
                        c->N, c->S, (nbp_likelihood_rec *)q.at(c, 0)));
  NBPCHK(q.fetch(c));
  for (int i = 0; i < n; i++) {
    loglik_out[i] = rec[i].loglik;
    if (comp_loglik_out)
      for (int k = 0; k < NBP_MAXC; k++) comp_loglik_out[(size_t)i * NBP_MAXC + k] = rec[i].comp_loglik[k];
  }
  return NBP_OK;
}

// the opening of both host-buffer forms: *p = the descriptor aimed at slot 0 (and 1: *unary false), checked as its batch form checks it
static nbp_status likelihood_host_desc(nbp_ctx *c, const char *who, const nbp_likelihood_desc *desc, const double *a, int32_t na,
                                       const double *b, int32_t nb, const void *out, nbp_likelihood_desc *p, bool *unary) {
  if (!c || !desc || !a || !out || (desc->kind != NBP_F_PRIOR && !b)) return fail(NBP_ERR_ARG, "null argument");
  *p = *desc;
  *unary = p->kind == NBP_F_PRIOR;
  p->slot_a = 0;
  p->slot_b = *unary ? -1 : 1;
  if (!*unary && c->n_slots < 2) return fail(NBP_ERR_RANGE, std::string(who) + ": the context needs two slots");
  NBPCHK(likelihood_check(c, p, 1));
  if (na < 0 || (!*unary && nb < 0)) return fail(NBP_ERR_ARG, std::string(who) + ": a negative count");
  return NBP_OK;
}

// host-buffer form: stages through slots 0 and 1 (which it clobbers), like nbp_kde_kld; the descriptor's own slots are not read
nbp_status nbp_factor_likelihood(nbp_ctx *c, const nbp_likelihood_desc *desc, const double *a, int32_t na, const double *b, int32_t nb,
                                 double *loglik_out, double *comp_loglik_out) {
  nbp_likelihood_desc p;
  bool unary;
  NBPCHK(likelihood_host_desc(c, "factor_likelihood", desc, a, na, b, nb, loglik_out, &p, &unary));
  if (na == 0 || (!unary && nb == 0)) {  // a belief without points: NaN, nothing launched
    *loglik_out = NAN;
    if (comp_loglik_out)
      for (int k = 0; k < NBP_MAXC; k++) comp_loglik_out[k] = NAN;
    return NBP_OK;
  }
  NBPCHK(kde_write(c, p.manifold, {{a, na, nullptr}, {unary ? nullptr : b, nb, nullptr}}));
  return nbp_run_factor_likelihood(c, &p, 1, loglik_out, comp_loglik_out);
}

// the same likelihood group by group (nbp_mode_likelihood_kernel): one upload of the descriptors, the row indices and the label rows,
// one launch, one copy back.  The query scratch holds table[n][8][8] | counts[n][2][8] (int32).
nbp_status nbp_run_factor_mode_likelihood(nbp_ctx *c, const nbp_likelihood_desc *descs, const int32_t *row_a, const int32_t *row_b, int32_t n,
                                          const int32_t *labels, int32_t n_rows, double *table_out, int32_t *counts_out) {
  if (!c || ((!descs || !row_a || !row_b || !table_out) && n > 0) || (n > 0 && n_rows > 0 && !labels)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  if (n_rows < 0) return fail(NBP_ERR_ARG, "factor_mode_likelihood: a negative number of label rows");
  NBPCHK(likelihood_check(c, descs, n));
  const size_t N = (size_t)c->N;
  std::vector<char> seen((size_t)n_rows, 0);
  for (int i = 0; i < n; i++) {
    const std::string who = "factor_mode_likelihood: item " + std::to_string(i) + ": ";
    if (row_a[i] < -1 || row_a[i] >= n_rows) return fail(NBP_ERR_RANGE, who + "row_a outside -1 .. n_rows - 1");
    if (row_b[i] < -1 || row_b[i] >= n_rows) return fail(NBP_ERR_RANGE, who + "row_b outside -1 .. n_rows - 1");
    if (descs[i].kind == NBP_F_PRIOR && row_b[i] != -1) return fail(NBP_ERR_ARG, who + "a prior is unary: row_b must be -1");
    for (int r : {row_a[i], row_b[i]}) {
      if (r < 0 || seen[(size_t)r]) continue;
      seen[(size_t)r] = 1;
      for (size_t k = 0; k < N; k++)
        if (labels[(size_t)r * N + k] < -1 || labels[(size_t)r * N + k] >= NBP_MAXK)
          return fail(NBP_ERR_ARG, "factor_mode_likelihood: label row " + std::to_string(r) + ": entry " + std::to_string(k) + " outside -1 .. NBP_MAXK - 1");
    }
  }
  const scratch_layout q{{sizeof(double), (size_t)n * NBP_MAXK * NBP_MAXK, table_out}, {4, (size_t)n * 2 * NBP_MAXK, counts_out}};
  const int32_t *d[4];
  NBPCHK(stage_columns(c, {{descs, sizeof(nbp_likelihood_desc) * (size_t)n}, {row_a, 4 * (size_t)n}, {row_b, 4 * (size_t)n},
                           {labels, 4 * (size_t)n_rows * N}}, d, q.total()));
  NBPCHK(launch_checked(c, nbp_mode_likelihood_kernel, n, c->Npad, nbp_mode_likelihood_lds_bytes(c->N), (const nbp_likelihood_desc *)d[0], d[1],
                        d[2], d[3], c->arena, c->N, c->S, q.at(c, 0), (int32_t *)q.at(c, 1)));
  return q.fetch(c);
}

// host-buffer form: stages through slots 0 and 1 (which it clobbers), like nbp_factor_likelihood; the label rows are padded with -1
nbp_status nbp_factor_mode_likelihood(nbp_ctx *c, const nbp_likelihood_desc *desc, const double *a, int32_t na, const int32_t *labels_a,
                                      const double *b, int32_t nb, const int32_t *labels_b, double *table_out, int32_t *counts_out) {
  nbp_likelihood_desc p;
  bool unary;
  NBPCHK(likelihood_host_desc(c, "factor_mode_likelihood", desc, a, na, b, nb, table_out, &p, &unary));
  const int N = c->N;
  std::vector<int32_t> rows;
  int32_t ra = -1, rb = -1, n_rows = 0;
  const auto row = [&](const int32_t *lab, int32_t cnt) {
    rows.resize((size_t)(n_rows + 1) * (size_t)N, -1);
    for (int i = 0; i < cnt && i < N; i++) rows[(size_t)n_rows * (size_t)N + i] = lab[i];
    return n_rows++;
  };
  if (labels_a) ra = row(labels_a, na);
  if (!unary && labels_b) rb = row(labels_b, nb);
  for (size_t k = 0; k < rows.size(); k++)
    if (rows[k] < -1 || rows[k] >= NBP_MAXK)
      return fail(NBP_ERR_ARG, "factor_mode_likelihood: label row " + std::to_string(k / (size_t)N) + ": entry " + std::to_string(k % (size_t)N) + " outside -1 .. NBP_MAXK - 1");
  if (na == 0 || (!unary && nb == 0)) {  // a belief without points: NaN, nothing launched
    for (int k = 0; k < NBP_MAXK * NBP_MAXK; k++) table_out[k] = NAN;
    if (counts_out)
      for (int k = 0; k < 2 * NBP_MAXK; k++) counts_out[k] = 0;
    return NBP_OK;
  }
  NBPCHK(kde_write(c, p.manifold, {{a, na, nullptr}, {unary ? nullptr : b, nb, nullptr}}));
  return nbp_run_factor_mode_likelihood(c, &p, &ra, &rb, 1, rows.data(), n_rows, table_out, counts_out);
}

// ---- local products on a grid (nbp_productgrid.h) ------------------------------------------------------------------------------
// what nbp_run_product_grid refuses: the items first (the measurement model through the factor likelihood's own check, with `other`
// in place of its slots), then descriptor by descriptor; nothing has been launched or written
static nbp_status product_grid_check(nbp_ctx *c, const nbp_product_grid_desc *descs, int n_desc, const nbp_product_item *items, int n_items,
                                     const int32_t *first) {
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n_items; i++) {
    const nbp_product_item &it = items[i];
    nbp_likelihood_desc p = it.lik;
    const bool unary = p.kind == NBP_F_PRIOR;
    refusal r{NBP_OK, nullptr};
    if (it.role != 0 && it.role != 1) r = {NBP_ERR_ARG, "role outside 0 / 1"};
    else if (unary && it.role == 1) r = {NBP_ERR_ARG, "role 1 on a unary item"};
    else if (unary && it.other != -1) r = {NBP_ERR_ARG, "a unary item has no other slot: other must be -1"};
    else if (!unary && (it.other < 0 || it.other >= c->n_slots)) r = {NBP_ERR_RANGE, "other slot out of range"};
    if (!r.what) {
      p.slot_a = unary ? 0 : it.other;
      p.slot_b = unary ? -1 : it.other;
      r = likelihood_item_refusal(c, p);
    }
    if (!r.what && (std::isnan(it.log_prior) || it.log_prior == INFINITY)) r = {NBP_ERR_ARG, "log_prior is NaN or +inf"};
    if (r.what) return fail(r.code, "product grid: item " + std::to_string(i) + ": " + r.what);
  }
  if (first[0] != 0) return fail(NBP_ERR_RANGE, "product grid: descriptor 0: first[0] must be 0");
  for (int i = 0; i < n_desc; i++) {
    const nbp_product_grid_desc &g = descs[i];
    const std::string who = "product grid: descriptor " + std::to_string(i) + ": ";
    if (!manifold_ok(g.manifold)) return fail(NBP_ERR_ARG, who + "unknown manifold");
    if (g.flags & ~NBP_PGRID_AUTO_EXTENT) return fail(NBP_ERR_ARG, who + "unknown flag");
    const bool autoext = g.flags & NBP_PGRID_AUTO_EXTENT;
    const int D = manifold_dim_h(g.manifold);
    if (autoext && (g.slot < 0 || g.slot >= c->n_slots)) return fail(NBP_ERR_RANGE, who + "slot out of range");
    if (autoext && !std::isfinite(g.margin)) return fail(NBP_ERR_RANGE, who + "margin not finite");
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
      if (g.n[a] < 1 || g.n[a] > NBP_GRID_MAX) return fail(NBP_ERR_RANGE, who + "n outside 1 .. " + std::to_string(NBP_GRID_MAX));
      if (a >= D && g.n[a] != 1) return fail(NBP_ERR_RANGE, who + "n must be 1 on an axis the manifold does not have");
      if (a < D && autoext && !manifold_circ_h(g.manifold, a) && g.n[a] < 2)
        return fail(NBP_ERR_RANGE, who + "automatic extent of a Euclidean axis needs n >= 2");
      if (a < D && !autoext && !std::isfinite(g.lo[a])) return fail(NBP_ERR_RANGE, who + "lo not finite");
      if (a < D && !autoext && !(g.step[a] > 0.0 && std::isfinite(g.step[a]))) return fail(NBP_ERR_RANGE, who + "step must be finite and positive");
      cells *= g.n[a];
    }
    if (cells > (int64_t)NBP_PGRID_MAX_CELLS) return fail(NBP_ERR_RANGE, who + "more than 2^22 cells");
    if (g.first_item < 0 || g.n_items < 0 || (int64_t)g.first_item + g.n_items > n_items) return fail(NBP_ERR_RANGE, who + "item range outside the list");
    for (int k = g.first_item; k < g.first_item + g.n_items; k++) {
      if (items[k].lik.manifold != g.manifold) return fail(NBP_ERR_ARG, who + "item " + std::to_string(k) + " lies on another manifold than the grid");
      if (k > g.first_item && items[k].group < items[k - 1].group)
        return fail(NBP_ERR_ARG, who + "item " + std::to_string(k) + ": groups must not decrease along the grid's items");
    }
    if ((int64_t)first[i + 1] - (int64_t)first[i] != cells) return fail(NBP_ERR_RANGE, who + "offsets do not match the grid size");
  }
  return NBP_OK;
}

// L(x) of any number of grids: the descriptors, the items, the offsets and the chunk table go up in one staging copy; the extents, one
// workgroup per chunk of 256 cells, the normalisation; the grids are copied straight into the caller's buffer, the records and the
// extents in one more copy (scratch_layout::fetch_split)
nbp_status nbp_run_product_grid(nbp_ctx *c, const nbp_product_grid_desc *descs, int32_t n_desc, const nbp_product_item *items, int32_t n_items,
                                const int32_t *first, double *logp_out, nbp_product_grid_rec *recs_out, double *extent_out) {
  if (!c || n_desc < 0 || n_items < 0 || ((!descs || !first) && n_desc > 0) || (!items && n_items > 0)) return fail(NBP_ERR_ARG, "product grid: null argument or a negative count");
  if (n_desc == 0) return NBP_OK;
  NBPCHK(product_grid_check(c, descs, n_desc, items, n_items, first));
  if (!logp_out) return fail(NBP_ERR_ARG, "product grid: null argument");
  std::vector<int32_t> chunks;
  for (int i = 0; i < n_desc; i++)
    for (int32_t k = 0; k < first[i + 1] - first[i]; k += NBP_PGRID_CHUNK) {
      chunks.push_back(i);
      chunks.push_back(k);
    }
  static_assert(sizeof(nbp_product_item) % 8 == 0 && sizeof(nbp_product_grid_desc) % 8 == 0, "the product-grid structs keep their doubles aligned in an array");
  static_assert(sizeof(nbp_product_grid_rec) == 24, "nbp_product_grid_rec fills three doubles of the query scratch");
  const size_t n = (size_t)n_desc, total = (size_t)first[n_desc];
  const scratch_layout q{{sizeof(nbp_product_grid_rec), n, recs_out}, {sizeof(double), 6 * n, extent_out}, {sizeof(double), total, logp_out}};
  const int32_t *d[4];
  NBPCHK(stage_columns(c, {{descs, sizeof(nbp_product_grid_desc) * n}, {items, sizeof(nbp_product_item) * (size_t)n_items}, {first, 4 * (n + 1)},
                           {chunks.data(), 4 * chunks.size()}}, d, q.total()));
  const nbp_product_grid_desc *dd = (const nbp_product_grid_desc *)d[0];
  NBPCHK(launch_checked(c, nbp_product_extent_kernel, n, 64, 0, dd, (const double *)c->arena, c->N, c->S, q.at(c, 1)));
  NBPCHK(launch_checked(c, nbp_product_fill_kernel, chunks.size() / 2, NBP_PGRID_CHUNK, nbp_product_fill_lds_bytes(c->N), dd,
                        (const nbp_product_item *)d[1], d[2], d[3], (const double *)q.at(c, 1), (const double *)c->arena, c->N, c->S, q.at(c, 2)));
  NBPCHK(launch_checked(c, nbp_product_norm_kernel, n, NBP_PGRID_CHUNK, 0, dd, d[2], (const double *)q.at(c, 1), (const double *)q.at(c, 2),
                        (nbp_product_grid_rec *)q.at(c, 0)));
  return q.fetch_split(c, 2);  // (the grids straight into the caller's buffer)
}

// host-buffer form for one grid: the variable's own belief through slot 0 (automatic extent only), the cloud of item k through slot
// 1 + k -- slots 0 .. n_items are clobbered; every refusal comes before the first write
nbp_status nbp_product_grid(nbp_ctx *c, const nbp_product_grid_desc *desc, const nbp_product_item *items, int32_t n_items,
                            const double *const *others, const int32_t *counts, const double *own, int32_t n_own, const double *own_bw,
                            double *logp_out, nbp_product_grid_rec *rec_out, double *extent_out) {
  if (!c || !desc || !logp_out || n_items < 0 || (n_items > 0 && (!items || !others || !counts))) return fail(NBP_ERR_ARG, "product grid: null argument or a negative count");
  nbp_product_grid_desc g = *desc;
  g.slot = 0;
  g.first_item = 0;
  g.n_items = n_items;
  const bool autoext = g.flags & NBP_PGRID_AUTO_EXTENT;
  if (autoext && (!own || !own_bw || n_own < 1)) return fail(NBP_ERR_ARG, "product grid: the automatic extent needs the variable's own points and bandwidth");
  if (c->n_slots < 1 + n_items) return fail(NBP_ERR_RANGE, "product grid: the context needs 1 + n_items slots");
  std::vector<nbp_product_item> its(items, items + n_items);
  for (int k = 0; k < n_items; k++) {
    const bool unary = its[k].lik.kind == NBP_F_PRIOR;
    its[k].other = unary ? -1 : 1 + k;
    if (!unary && (!others[k] || counts[k] < 1)) return fail(NBP_ERR_ARG, "product grid: item " + std::to_string(k) + ": a belief holds at least one point");
  }
  int64_t cells = 1;
  for (int a = 0; a < 3; a++) cells *= std::max(g.n[a], 0);
  const int32_t first[2] = {0, (int32_t)std::min<int64_t>(cells, INT32_MAX)};
  NBPCHK(product_grid_check(c, &g, 1, its.data(), n_items, first));  // (before a slot is touched)
  const double ones[NBP_MAXD] = {1.0, 1.0, 1.0};
  if (autoext) NBPCHK(nbp_belief_write(c, 0, g.manifold, own, n_own, own_bw, nullptr));
  for (int k = 0; k < n_items; k++)
    if (its[k].other >= 0) NBPCHK(nbp_belief_write(c, its[k].other, g.manifold, others[k], counts[k], ones, nullptr));
  return nbp_run_product_grid(c, &g, 1, its.data(), n_items, first, logp_out, rec_out, extent_out);
}

// ---- heatmap densities (nbp_heatmap.h) -------------------------------------------------------------------------------------------
struct nbp_heatmap {
  nbp_ctx *ctx = nullptr;  // null: the context was destroyed
  int nx = 0, ny = 0, M = 0;
  double h = 0, dx = 0, dy = 0, total = 0, wtotal = 0;
  double *data = nullptr, *x = nullptr, *y = nullptr, *cdf = nullptr, *t2 = nullptr, *p2 = nullptr;  // field, axes, scan(w), tile totals
  int *lastpos = nullptr;                                                                              // last cell with w > 0 ...
  int lastpos_h = -1;                                                                                  // ... as the host found it
  int cap = 0;                                                                                         // pre-samples the buffers below hold
  int32_t *cell = nullptr;
  double2 *pre = nullptr;
  double *d = nullptr, *W = nullptr, *wcdf = nullptr, *wt2 = nullptr, *wp2 = nullptr;
  unsigned long long *dmin_key = nullptr;
  int dcap = 0;  // drawn points the buffers below hold
  int32_t *pick = nullptr;
  double2 *pts = nullptr;
};
static void heatmap_free_pre(nbp_heatmap *hm) {
  for (void *p : {(void *)hm->cell, (void *)hm->pre, (void *)hm->d, (void *)hm->W, (void *)hm->wcdf, (void *)hm->wt2, (void *)hm->wp2})
    if (p) hipFree(p);
  hm->cell = nullptr; hm->pre = nullptr; hm->d = hm->W = hm->wcdf = hm->wt2 = hm->wp2 = nullptr;
  hm->cap = hm->M = 0;
}
static void heatmap_release(nbp_heatmap *hm) {
  nbp_ctx *c = hm->ctx;
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  heatmap_free_pre(hm);
  for (void *p : {(void *)hm->data, (void *)hm->x, (void *)hm->y, (void *)hm->cdf, (void *)hm->t2, (void *)hm->p2, (void *)hm->lastpos,
                  (void *)hm->dmin_key, (void *)hm->pick, (void *)hm->pts})
    if (p) hipFree(p);
  hm->data = hm->x = hm->y = hm->cdf = hm->t2 = hm->p2 = nullptr;
  hm->lastpos = nullptr; hm->dmin_key = nullptr; hm->pick = nullptr; hm->pts = nullptr;
  hm->dcap = 0;
  c->heatmaps.erase(std::remove(c->heatmaps.begin(), c->heatmaps.end(), hm), c->heatmaps.end());
  hm->ctx = nullptr;
}
// scan(in) -> out (nbp_heatmap.h: totals, tiles, apply), n <= NBP_HM_MAX_CELLS checked by the callers
static nbp_status heatmap_scan(nbp_ctx *c, const double *in, int n, double *t2, double *p2, double *out) {
  const size_t tiles = ((size_t)n + NBP_HM_TILE - 1) / NBP_HM_TILE;
  NBPCHK(launch_checked(c, nbp_hm_scan_totals_kernel, tiles, NBP_HM_LANES, 0, in, n, t2));
  NBPCHK(launch_checked(c, nbp_hm_scan_tiles_kernel, 1, NBP_HM_LANES, 0, (const double *)t2, (int)tiles, p2));
  return launch_checked(c, nbp_hm_scan_apply_kernel, tiles, NBP_HM_LANES, 0, in, n, (const double *)t2, (const double *)p2, out);
}
// dx of the definition and the refusal of an axis that is not strictly increasing and uniform to 1e-9 of its spacing
static bool heatmap_axis(const double *x, int n, double *dx) {
  const double s = (x[n - 1] - x[0]) / (double)(n - 1);
  if (!(std::isfinite(x[0]) && std::isfinite(s) && s > 0.0)) return false;
  for (int i = 0; i + 1 < n; i++)
    if (!(x[i + 1] > x[i]) || !(std::fabs((x[i + 1] - x[i]) - s) <= 1e-9 * std::fabs(s))) return false;
  *dx = s;
  return true;
}

nbp_status nbp_heatmap_create(nbp_ctx *c, const double *data, int32_t nx, int32_t ny, const double *x, const double *y, double bw_factor,
                              nbp_heatmap **out) {
  if (!c || !out) return fail(NBP_ERR_ARG, "null argument");
  *out = nullptr;
  if (nx < 2 || ny < 2) return fail(NBP_ERR_INVALID, "heatmap: nx, ny >= 2");
  if ((int64_t)nx * (int64_t)ny > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap: more than 2^26 cells");
  if (!data || !x || !y) return fail(NBP_ERR_ARG, "null argument");
  if (!(std::isfinite(bw_factor) && bw_factor > 0.0)) return fail(NBP_ERR_INVALID, "heatmap: bw_factor must be positive and finite");
  double dx = 0, dy = 0;
  if (!heatmap_axis(x, nx, &dx)) return fail(NBP_ERR_INVALID, "heatmap: x is not strictly increasing with uniform spacing");
  if (!heatmap_axis(y, ny, &dy)) return fail(NBP_ERR_INVALID, "heatmap: y is not strictly increasing with uniform spacing");
  const int n = nx * ny;
  bool finite = true;
  int lastpos = -1;  // the last cell with w > 0
  for (int i = 0; i < n; i++) {
    finite &= std::isfinite(data[i]);
    lastpos = data[i] > 0.0 ? i : lastpos;
  }
  if (!finite) return fail(NBP_ERR_INVALID, "heatmap: the field holds a value that is not finite");
  if (lastpos < 0) return fail(NBP_ERR_INVALID, "heatmap: no positive cell");
  const double h = bw_factor * 0.5 * (dx + dy);
  if (!(std::isfinite(h) && h > 0.0)) return fail(NBP_ERR_INVALID, "heatmap: the bandwidth is not positive and finite");
  HIPCHK(hipSetDevice(c->device));
  nbp_heatmap *hm = new nbp_heatmap;
  hm->ctx = c;
  hm->nx = nx; hm->ny = ny; hm->dx = dx; hm->dy = dy; hm->h = h; hm->lastpos_h = lastpos;
  c->heatmaps.push_back(hm);
  const size_t tiles = ((size_t)n + NBP_HM_TILE - 1) / NBP_HM_TILE;
  auto body = [&]() -> nbp_status {
    HIPCHK(hipMalloc(&hm->data, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc(&hm->cdf, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc(&hm->x, sizeof(double) * (size_t)nx));
    HIPCHK(hipMalloc(&hm->y, sizeof(double) * (size_t)ny));
    HIPCHK(hipMalloc(&hm->t2, sizeof(double) * tiles));
    HIPCHK(hipMalloc(&hm->p2, sizeof(double) * tiles));
    HIPCHK(hipMalloc(&hm->lastpos, sizeof(int)));
    HIPCHK(hipMalloc(&hm->dmin_key, sizeof(unsigned long long)));
    HIPCHK(hipMemcpyAsync(hm->data, data, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(hm->x, x, sizeof(double) * (size_t)nx, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(hm->y, y, sizeof(double) * (size_t)ny, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(hm->lastpos, &hm->lastpos_h, sizeof(int), hipMemcpyHostToDevice, c->stream));
    NBPCHK(heatmap_scan(c, hm->data, n, hm->t2, hm->p2, hm->cdf));
    HIPCHK(hipMemcpyAsync(&hm->total, hm->cdf + (n - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!(std::isfinite(hm->total) && hm->total > 0.0)) return fail(NBP_ERR_INVALID, "heatmap: the sum of the positive cells is not positive and finite");
    return NBP_OK;
  };
  const nbp_status rc = body();
  if (rc) {
    const std::string msg = g_err;
    heatmap_release(hm);
    delete hm;
    return fail(rc, msg);
  }
  *out = hm;
  return NBP_OK;
}

nbp_status nbp_heatmap_build(nbp_heatmap *hm, int32_t M, uint64_t seed, int32_t *cell_M, double *pre_Mx2, double *d_M, double *W_M) {
  if (!hm) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx *c = hm->ctx;
  if (!c) return fail(NBP_ERR_ARG, "heatmap: the context was destroyed");
  if (M < 1 || M > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap build: M outside 1 .. 2^26");
  HIPCHK(hipSetDevice(c->device));
  hm->M = 0;  // (a build that fails leaves no pre-samples)
  hm->wtotal = 0;
  if (M > hm->cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    heatmap_free_pre(hm);
    const size_t tiles = ((size_t)M + NBP_HM_TILE - 1) / NBP_HM_TILE;
    HIPCHK(hipMalloc(&hm->cell, sizeof(int32_t) * (size_t)M));
    HIPCHK(hipMalloc(&hm->pre, sizeof(double2) * (size_t)M));
    HIPCHK(hipMalloc(&hm->d, sizeof(double) * (size_t)M));
    HIPCHK(hipMalloc(&hm->W, sizeof(double) * (size_t)M));
    HIPCHK(hipMalloc(&hm->wcdf, sizeof(double) * (size_t)M));
    HIPCHK(hipMalloc(&hm->wt2, sizeof(double) * tiles));
    HIPCHK(hipMalloc(&hm->wp2, sizeof(double) * tiles));
    hm->cap = M;
  }
  const size_t blocks = ((size_t)M + NBP_HM_LANES - 1) / NBP_HM_LANES;
  HIPCHK(hipMemsetAsync(hm->dmin_key, 0xFF, sizeof(unsigned long long), c->stream));
  NBPCHK(launch_checked(c, nbp_hm_presample_kernel, blocks, NBP_HM_LANES, 0, (const double *)hm->data, (const double *)hm->x,
                        (const double *)hm->y, (const double *)hm->cdf, (const int *)hm->lastpos, hm->nx, hm->ny, hm->dx, hm->dy, hm->h,
                        (int)M, seed, hm->cell, hm->pre, hm->d, hm->dmin_key));
  NBPCHK(launch_checked(c, nbp_hm_weight_kernel, blocks, NBP_HM_LANES, 0, (const double *)hm->d, (const unsigned long long *)hm->dmin_key,
                        (int)M, hm->W));
  NBPCHK(heatmap_scan(c, hm->W, M, hm->wt2, hm->wp2, hm->wcdf));
  HIPCHK(hipMemcpyAsync(&hm->wtotal, hm->wcdf + (M - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cell_M) HIPCHK(hipMemcpyAsync(cell_M, hm->cell, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  if (pre_Mx2) HIPCHK(hipMemcpyAsync(pre_Mx2, hm->pre, sizeof(double2) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  if (d_M) HIPCHK(hipMemcpyAsync(d_M, hm->d, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  if (W_M) HIPCHK(hipMemcpyAsync(W_M, hm->W, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  hm->M = M;
  return NBP_OK;
}

nbp_status nbp_heatmap_draw(nbp_heatmap *hm, int32_t n, uint64_t seed, int32_t jitter, int32_t slot, int32_t *pick_n, double *pts_nx2,
                            double *bw_2) {
  if (!hm) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx *c = hm->ctx;
  if (!c) return fail(NBP_ERR_ARG, "heatmap: the context was destroyed");
  if (hm->M < 1) return fail(NBP_ERR_INVALID, "heatmap draw: no pre-samples (nbp_heatmap_build comes first)");
  if (n < 1 || n > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap draw: n outside 1 .. 2^26");
  if (slot < -1 || slot >= c->n_slots) return fail(NBP_ERR_RANGE, "heatmap draw: slot out of range");
  if (slot >= 0 && n > c->N) return fail(NBP_ERR_INVALID, "heatmap draw: a slot holds at most N points");
  HIPCHK(hipSetDevice(c->device));
  if (n > hm->dcap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (hm->pick) HIPCHK(hipFree(hm->pick));
    if (hm->pts) HIPCHK(hipFree(hm->pts));
    hm->pick = nullptr; hm->pts = nullptr; hm->dcap = 0;
    HIPCHK(hipMalloc(&hm->pick, sizeof(int32_t) * (size_t)n));
    HIPCHK(hipMalloc(&hm->pts, sizeof(double2) * (size_t)n));
    hm->dcap = n;
  }
  double *s = slot >= 0 ? c->arena + c->S * slot : nullptr;
  if (s) HIPCHK(hipMemsetAsync(s, 0, sizeof(double) * (size_t)c->S, c->stream));
  NBPCHK(launch_checked(c, nbp_hm_draw_kernel, ((size_t)n + NBP_HM_LANES - 1) / NBP_HM_LANES, NBP_HM_LANES, 0, (const double *)hm->wcdf,
                        (const double2 *)hm->pre, hm->M, hm->h, (int)n, seed, (int)(jitter != 0), hm->pick, hm->pts, s, c->N));
  if (pick_n) HIPCHK(hipMemcpyAsync(pick_n, hm->pick, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (pts_nx2) HIPCHK(hipMemcpyAsync(pts_nx2, hm->pts, sizeof(double2) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (pick_n || pts_nx2) HIPCHK(hipStreamSynchronize(c->stream));
  if (bw_2) bw_2[0] = bw_2[1] = hm->h;
  return NBP_OK;
}

nbp_status nbp_heatmap_info(const nbp_heatmap *hm, double *bw_2, double *total, double *wtotal, int32_t *M) {
  if (!hm) return fail(NBP_ERR_ARG, "null argument");
  if (bw_2) bw_2[0] = bw_2[1] = hm->h;
  if (total) *total = hm->total;
  if (wtotal) *wtotal = hm->wtotal;
  if (M) *M = hm->M;
  return NBP_OK;
}

nbp_status nbp_heatmap_destroy(nbp_heatmap *hm) {
  if (!hm) return NBP_OK;
  heatmap_release(hm);
  delete hm;
  return NBP_OK;
}

// ---- self-tests of SCAN and SEARCH (nbp_heatmap.h): the whole scan and the search at given probes, back on the host ---------------
nbp_status nbp_heatmap_scan_eval(nbp_ctx *c, const double *in, int32_t n, double *out) {
  if (!c) return fail(NBP_ERR_ARG, "null argument");
  if (n < 1 || n > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap scan_eval: n outside 1 .. 2^26");
  if (!in || !out) return fail(NBP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  const size_t tiles = ((size_t)n + NBP_HM_TILE - 1) / NBP_HM_TILE;
  double *d_in = nullptr, *d_out = nullptr, *t2 = nullptr, *p2 = nullptr;
  auto body = [&]() -> nbp_status {
    HIPCHK(hipMalloc(&d_in, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc(&d_out, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc(&t2, sizeof(double) * tiles));
    HIPCHK(hipMalloc(&p2, sizeof(double) * tiles));
    HIPCHK(hipMemcpyAsync(d_in, in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    NBPCHK(heatmap_scan(c, d_in, n, t2, p2, d_out));
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NBP_OK;
  };
  const nbp_status rc = body();
  if (rc) hipStreamSynchronize(c->stream);  // (nothing of the stream may still read what is freed below)
  for (void *p : {(void *)d_in, (void *)d_out, (void *)t2, (void *)p2})
    if (p) hipFree(p);
  return rc;
}

nbp_status nbp_heatmap_search_eval(nbp_ctx *c, const double *cdf, int32_t n, const double *t, int32_t nt, int32_t *idx_out) {
  if (!c) return fail(NBP_ERR_ARG, "null argument");
  if (n < 1 || n > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap search_eval: n outside 1 .. 2^26");
  if (nt < 1 || nt > NBP_HM_MAX_CELLS) return fail(NBP_ERR_INVALID, "heatmap search_eval: nt outside 1 .. 2^26");
  if (!cdf || !t || !idx_out) return fail(NBP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  double *d_cdf = nullptr, *d_t = nullptr;
  int32_t *d_idx = nullptr;
  auto body = [&]() -> nbp_status {
    HIPCHK(hipMalloc(&d_cdf, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc(&d_t, sizeof(double) * (size_t)nt));
    HIPCHK(hipMalloc(&d_idx, sizeof(int32_t) * (size_t)nt));
    HIPCHK(hipMemcpyAsync(d_cdf, cdf, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_t, t, sizeof(double) * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    NBPCHK(launch_checked(c, nbp_hm_search_eval_kernel, ((size_t)nt + NBP_HM_LANES - 1) / NBP_HM_LANES, NBP_HM_LANES, 0,
                          (const double *)d_cdf, (int)n, (const double *)d_t, (int)nt, d_idx));
    HIPCHK(hipMemcpyAsync(idx_out, d_idx, sizeof(int32_t) * (size_t)nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NBP_OK;
  };
  const nbp_status rc = body();
  if (rc) hipStreamSynchronize(c->stream);
  for (void *p : {(void *)d_cdf, (void *)d_t, (void *)d_idx})
    if (p) hipFree(p);
  return rc;
}

nbp_status nbp_run_resample(nbp_ctx *c, const int32_t *slots, const int32_t *manifolds, int32_t n, uint64_t seed) {
  if (!c || ((!slots || !manifolds) && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (n <= 0) return NBP_OK;
  NBPCHK(batch_check(c, "resample", {slots}, manifolds, n, no_refusal));
  const int32_t *d[2];
  NBPCHK(stage_columns(c, {{slots, 4 * (size_t)n}, {manifolds, 4 * (size_t)n}}, d, 0));
  NBPCHK(launch_checked(c, nbp_resample_kernel, n, 256, 0, d[0], d[1], c->arena, c->N, c->S, seed));
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBP_OK;
}

// ---- resident programs ---------------------------------------------------------------------------------
// Scheduling of the bandwidth fits (manikde!).  Fits are *deferred*: a proposal stage only queues
// its fits; the next product stage runs them inside its nbp_prep_kernel launch, next to the KD-tree
// builds (which need points, not bandwidths); the product's own rebandwidth is queued in turn and
// rides with the prep launch of the NEXT update.  A queued fit is flushed early (plain
// nbp_bandwidth_kernel launch) when a later stage reads the bandwidth of that slot: a MsgPrior
// proposal sampling from it, or a copy stage moving whole slots.  Per update the critical path is
// proposal -> prep (LCV || KD) -> product.
// nbp_program_finalize compiles the stages in named steps: plan_sinks (which update of the up pass runs in a later stage),
// plan_lanes (lane 1's descriptors and the leaving ones behind the others), gather_sinks (the gathered copies a sink stage
// runs), plan_pipeline (reorders the descriptors of a round into its two halves), product_liveness, schedule_fits (the walk
// over the pending fits; schedule_fused_pair where a round runs as one launch), split_piped_entry_fits, plan_parts,
// layout_blob, presize, acquire_device_blob, upload_blob.  What a stage of any kind reads and writes they all learn from
// one walk, stage_reads / stage_writes.
struct nbp_stage {
  int kind = 0, n = 0, maxfd = 0, mani = 0;  // mani: products_uniform_manifold / proposals_uniform_class
  size_t offset = 0;            // byte offset of the descriptors in the program blob
  nbp_fits ent;                 // fits pending at ENTRY of the stage
  bool flush_before = false;    // run the pending fits in a plain bandwidth launch before the stage
  bool need_prep = true;        // products: some product multiplies > 1 densities (KD builds; the entry fits run beside them)
  // fused variable updates: this PROPOSALS stage and the PRODUCTS stage behind it run as ONE nbp_update_kernel launch
  // (fused_second marks that PRODUCTS stage); upd = one nbp_update_desc per product
  bool fused = false, fused_second = false;
  int upd_F = 0;
  std::vector<nbp_update_desc> upd;
  size_t upd_off = 0;
  // a range of nbp_program_run that ends or starts BETWEEN the two stages of a fused pair runs them in the three-launch
  // form (run_range): the fused_second stage keeps, as its entry fits, the proposals of the pair that carry a bandwidth
  // and, here, the outputs the fused launch fits itself
  nbp_fits split_out;
  // two-stream round (plan_pipeline): descriptors [0, pipe_split) are the first half; on the PRODUCTS stage pipe_ent splits
  // the entry fits the same way.  `pipe` on the PROPOSALS stage = the pair runs that way.
  bool pipe = false;
  int pipe_split = -1, pipe_ent = 0;
  // where plan_pipeline put the descriptor the caller gave as the i-th of the stage (empty: where it was).  The seed table is
  // laid out through it (layout_blob): nbp_program_set_seeds takes its seeds in the CALLER's order
  std::vector<int> moved_to;
  // lanes (plan_lanes): the hint as nbp_program_set_lanes gave it (caller order); descriptors [lane_split, n) are lane 1
  // (-1: the stage has none)
  std::vector<int32_t> lane_hint;
  int lane_split = -1;
  // sinks (plan_sinks / gather_sinks).  sink_to: per descriptor in the caller's order the stage it runs in (empty: every one
  // in its own); plan_lanes puts the lane-0 descriptors that leave behind those that stay: [0, sink_stay) stay (-1: none
  // leaves).  A stage that gains descriptors has a gathered copy of its remaining lane-0 descriptors and the gained ones in
  // the blob: gather_n of them at gather_off, copied from (stage, place in that stage) gather_src; `gained` of them came
  // from other stages.  The descriptors of the stage itself stay whole where they are, for the runs that execute stages
  // whole.  On a part: the part runs such a copy.
  std::vector<int> sink_to;
  int sink_stay = -1;
  size_t gather_off = 0;
  int gather_n = 0, gained = 0;
  std::vector<std::pair<int, int>> gather_src;
  bool sink_touched = false, gathered = false;
  // as a PART of a program with lanes (nbp_program::parts): the lane, the stage it is a share of, every fit still pending
  // on either lane where its stage begins (`bound`, on the first part of a stage: what a range that ends there runs), the
  // parts of the other lane it waits for and whether one of them waits for it (nbp_lanes.h)
  int lane = 0, user = -1;
  nbp_fits bound;
  std::vector<int> waits;
  bool signals = false;
};
struct nbp_program {
  nbp_ctx *ctx = nullptr;
  std::vector<nbp_stage> stages;  // + one trailing pseudo stage holding the fits pending at exit
  std::vector<char> blob;
  char *dev = nullptr;
  size_t dev_bytes = 0;
  bool finalized = false;
  bool lazy_bw = false;  // NBP_OPT_LAZY_BANDWIDTH
  bool use_graph = true; // NBP_OPT_GRAPH_REPLAY
  bool use_fused = true; // NBP_OPT_FUSED_UPDATES
  bool async_upload = false;  // NBP_OPT_ASYNC_UPLOAD: the descriptor blob travels stream-ordered from a pinned buffer, nothing waits
  int n_user_stages = 0;
  // captured launch sequences of nbp_program_run(first, last): key = first * 2^32 + last
  struct captured { hipGraphExec_t exec; uint64_t ws_gen; };  // ws_gen: the context's workspace generation at capture time
  std::unordered_map<uint64_t, captured> graphs;
  std::unordered_map<uint64_t, int> runs;
  size_t seed_off = 0;  // table of the blob offsets of every descriptor's seed field (one reseed launch)
  size_t seed_val_off = 0;  // n_seeds values behind the table: where nbp_program_set_seeds puts the new seeds before it scatters them
  int n_seeds = 0;
  std::vector<int32_t> seed_rank;  // nbp_program_seed_order
  // lanes: the parts in list order + a trailing pseudo part (empty: the program has no lane 1); first_part[s] = the first
  // part of stage s (n_user_stages + 1 entries); what lane 1 needs of the KD workspace and of the statistics area
  std::vector<nbp_stage> parts;
  std::vector<int> first_part;
  size_t lane_ws = 0, lane_gstats = 0;
  // sinks: the option; whether the parts are built from the moved list; per sink the stages [first, last] its updates span
  // (a range that starts or ends inside runs the stages whole); behind the seed table the seed fields of the gathered
  // copies, n_dup of them, and behind the values the entry of the table each one follows (layout_blob)
  bool sinks = false;  // NBP_OPT_UP_PASS_SINKS
  bool sunk = false;
  std::vector<std::pair<int, int>> sink_regions;
  size_t dup_src_off = 0;
  int n_dup = 0;
};

nbp_status nbp_program_create(nbp_ctx *c, nbp_program **out) {
  if (!c || !out) return fail(NBP_ERR_ARG, "null argument");
  nbp_program *p = new nbp_program();
  p->ctx = c;
  c->programs.push_back(p);
  *out = p;
  return NBP_OK;
}
// the context is going away: free the device blob while the context's device is still current
static void program_detach(nbp_program *p) {
  for (auto &kv : p->graphs) hipGraphExecDestroy(kv.second.exec);
  p->graphs.clear();
  if (p->dev) hipFree(p->dev);
  p->dev = nullptr;
  p->ctx = nullptr;
}
static void program_delete(nbp_program *p) {
  program_detach(p);
  delete p;
}
#define PROG_ALIVE(p) do { if (!(p)->ctx) return fail(NBP_ERR_ARG, "the program's context was destroyed"); } while (0)

nbp_status nbp_program_add_stage(nbp_program *p, int32_t kind, const void *descs, int32_t n) {
  if (!p || (!descs && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  PROG_ALIVE(p);
  if (p->finalized) return fail(NBP_ERR_ARG, "program already finalized");
  if (n < 0) return fail(NBP_ERR_ARG, "n < 0");
  size_t esz;
  nbp_status rc = NBP_OK;
  nbp_stage st;
  switch (kind) {
  case NBP_STAGE_PROPOSALS:
    esz = sizeof(nbp_proposal_desc);
    rc = check_proposals(p->ctx, (const nbp_proposal_desc *)descs, n);
    st.mani = proposals_uniform_class((const nbp_proposal_desc *)descs, n);
    break;
  case NBP_STAGE_PRODUCTS:
    esz = sizeof(nbp_product_desc);
    rc = check_products(p->ctx, (const nbp_product_desc *)descs, n);
    st.maxfd = products_maxfd((const nbp_product_desc *)descs, n);
    st.mani = products_uniform_manifold((const nbp_product_desc *)descs, n);
    break;
  case NBP_STAGE_COPIES:
  case NBP_STAGE_COPY_POINTS: esz = sizeof(nbp_copy_desc); rc = check_copies(p->ctx, (const nbp_copy_desc *)descs, n); break;
  case NBP_STAGE_DECONV: esz = sizeof(nbp_proposal_desc); rc = check_deconv(p->ctx, (const nbp_proposal_desc *)descs, n); break;
  default: return fail(NBP_ERR_ARG, "unknown stage kind");
  }
  if (rc) return rc;
  size_t off = (p->blob.size() + 63) & ~(size_t)63;
  p->blob.resize(off + esz * (size_t)n);
  if (n) memcpy(p->blob.data() + off, descs, esz * (size_t)n);
  st.kind = kind; st.n = n; st.offset = off;
  p->stages.push_back(st);
  return NBP_OK;
}

// A hint, not an order: descriptor i of the stage may run on lane lane_of_descriptor[i] (0: the library stream, 1: the second
// stream), beside whatever the other lane runs meanwhile.  What a lane waits for is derived from the slots (plan_lanes).
nbp_status nbp_program_set_lanes(nbp_program *p, int32_t stage, const int32_t *lane_of_descriptor, int32_t n) {
  if (!p || (!lane_of_descriptor && n > 0)) return fail(NBP_ERR_ARG, "null argument");
  PROG_ALIVE(p);
  if (p->finalized) return fail(NBP_ERR_ARG, "program already finalized");
  if (stage < 0 || stage >= (int)p->stages.size()) return fail(NBP_ERR_RANGE, "set_lanes: no such stage");
  nbp_stage &st = p->stages[(size_t)stage];
  if (n != st.n) return fail(NBP_ERR_ARG, "set_lanes: one lane per descriptor of the stage");
  for (int i = 0; i < n; i++)
    if (lane_of_descriptor[i] != 0 && lane_of_descriptor[i] != 1) return fail(NBP_ERR_RANGE, "set_lanes: a lane is 0 or 1");
  st.lane_hint.assign(lane_of_descriptor, lane_of_descriptor + n);
  return NBP_OK;
}

nbp_status nbp_program_set_option(nbp_program *p, int32_t option, int32_t value) {
  if (!p) return fail(NBP_ERR_ARG, "null argument");
  // (graph replay is a property of the runs, not of the compiled stages: it may be switched after nbp_program_finalize --
  //  graphs already captured stay with the program and are used again when it is switched back on)
  if (option == NBP_OPT_GRAPH_REPLAY && p->finalized) { p->use_graph = value != 0; return NBP_OK; }
  if (p->finalized) return fail(NBP_ERR_ARG, "program already finalized");
  // NBP_NO_LAZY_BANDWIDTH=1 (environment): every fit the reference makes is made, whatever the program asks for -- the
  // measurement of what the option saves (bench.py "ms_per_step_every_fit")
  if (option == NBP_OPT_LAZY_BANDWIDTH) { p->lazy_bw = value != 0 && getenv("NBP_NO_LAZY_BANDWIDTH") == nullptr; return NBP_OK; }
  if (option == NBP_OPT_GRAPH_REPLAY) { p->use_graph = value != 0; return NBP_OK; }
  if (option == NBP_OPT_FUSED_UPDATES) { p->use_fused = value != 0; return NBP_OK; }
  if (option == NBP_OPT_ASYNC_UPLOAD) { p->async_upload = value != 0; return NBP_OK; }
  if (option == NBP_OPT_UP_PASS_SINKS) { p->sinks = value != 0; return NBP_OK; }
  return fail(NBP_ERR_ARG, "unknown program option");
}

// What the descriptors of a stage read and write, slot by slot: stage_reads / stage_writes, the one place that knows their
// anatomy (product_liveness, fused_plan, plan_pipeline and schedule_fits ask it).  What a read takes from its slot:
enum nbp_access {
  NBP_RD_POINTS,  // the points only: the variables of a factor, a product's old_slot, COPY_POINTS, a deconvolution's variables
  NBP_RD_KDE,     // points and bandwidth: the density a MsgPrior / pass-through proposal takes (var_slot[1]), a measurement
                  // KDE, an input of a real product, the source of a whole-slot copy
  NBP_RD_CARRY    // the single input of a pass-through product: the points, and whatever bandwidth the slot has (fitted or
                  // still pending) moves to the output with them
};
extern "C++" {  // (templates)
template <class F>  // f(slot, access)
static void proposal_reads(const nbp_proposal_desc &d, F &&f) {
  for (int k = 0; k < d.nvars; k++) f(d.var_slot[k], NBP_RD_POINTS);
  if (d.factor_kind == NBP_F_MSGPRIOR || d.factor_kind == NBP_F_PASSTHROUGH) f(d.var_slot[1], NBP_RD_KDE);  // (unary: nvars = 1)
  if (d.meas_kde > 0) f(d.meas_kde - 1, NBP_RD_KDE);
}
// f(descriptor, slot, access).  idle_old: also the old_slot of a pass-through product, which no kernel reads (fused_plan
// has always counted it: DESIGN.md 3)
template <class F>
static void stage_reads(const nbp_program *p, const nbp_stage &st, F &&f, bool idle_old = false) {
  const char *d = p->blob.data() + st.offset;
  for (int i = 0; i < st.n; i++)
    if (st.kind == NBP_STAGE_PROPOSALS || st.kind == NBP_STAGE_DECONV) {
      proposal_reads(((const nbp_proposal_desc *)d)[i], [&](int32_t slot, nbp_access a) { f(i, slot, a); });
    } else if (st.kind == NBP_STAGE_PRODUCTS) {
      const nbp_product_desc &q = ((const nbp_product_desc *)d)[i];
      for (int j = 0; j < q.nfactors; j++) f(i, q.in_slot[j], q.nfactors > 1 ? NBP_RD_KDE : NBP_RD_CARRY);
      if (q.old_slot >= 0 && (q.nfactors > 1 || idle_old)) f(i, q.old_slot, NBP_RD_POINTS);
    } else if (st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS) {
      f(i, ((const nbp_copy_desc *)d)[i].src_slot, st.kind == NBP_STAGE_COPIES ? NBP_RD_KDE : NBP_RD_POINTS);
    }
}
template <class F>  // f(descriptor, slot)
static void stage_writes(const nbp_program *p, const nbp_stage &st, F &&f) {
  const char *d = p->blob.data() + st.offset;
  for (int i = 0; i < st.n; i++)
    if (st.kind == NBP_STAGE_PROPOSALS || st.kind == NBP_STAGE_DECONV) f(i, ((const nbp_proposal_desc *)d)[i].out_slot);
    else if (st.kind == NBP_STAGE_PRODUCTS) f(i, ((const nbp_product_desc *)d)[i].out_slot);
    else if (st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS) f(i, ((const nbp_copy_desc *)d)[i].dst_slot);
}
// The same for the planners that order launches (plan_sinks, the lane sweep of plan_parts): rd(descriptor, x), wr(descriptor, x)
// with the points and the bandwidth of a slot apart (x = 2 * slot, 2 * slot + 1), an old_slot counted also where no kernel
// reads it, and the side buffer (hypothesis indices, labels) as one slot.
#define NBP_LANE_SLOT_SIDE (-2)
template <class R, class W>
static void stage_touches(const nbp_program *p, const nbp_stage &st, R &&rd, W &&wr) {
  stage_reads(p, st, [&](int i, int32_t slot, nbp_access acc) {
    rd(i, 2 * slot);
    if (acc != NBP_RD_POINTS || st.kind == NBP_STAGE_PRODUCTS) rd(i, 2 * slot + 1);
    if (acc == NBP_RD_POINTS && st.kind == NBP_STAGE_PRODUCTS) wr(i, 2 * slot);  // (old_slot: topped up in place)
  }, true);
  stage_writes(p, st, [&](int i, int32_t slot) {
    wr(i, 2 * slot);
    if (st.kind != NBP_STAGE_COPY_POINTS) wr(i, 2 * slot + 1);
  });
  const char *d = p->blob.data() + st.offset;
  for (int i = 0; i < st.n; i++)
    if (st.kind == NBP_STAGE_PROPOSALS || st.kind == NBP_STAGE_DECONV) {
      const nbp_proposal_desc &q = ((const nbp_proposal_desc *)d)[i];
      if (q.mhidx_in >= 0) rd(i, NBP_LANE_SLOT_SIDE);
      if (q.mhidx_out >= 0) wr(i, NBP_LANE_SLOT_SIDE);
    } else if (st.kind == NBP_STAGE_PRODUCTS && ((const nbp_product_desc *)d)[i].labels_out >= 0) {
      wr(i, NBP_LANE_SLOT_SIDE);
    }
}
}  // extern "C++"

// Liveness of product rebandwidths (NBP_OPT_LAZY_BANDWIDTH): the bandwidth of a product's output is read
// only by a MsgPrior proposal sampling that slot, by a product taking it as input, and by slot copies
// (which carry it along).  dead[s][i] = the output of product i of stage s is overwritten by a later
// product / copy / proposal before any of those happens, so its fit can be skipped without changing any
// result.  An EMPTY copy stage is a barrier ("everything may be read now": slots leave the device).
struct nbp_liveness {
  std::vector<std::vector<char>> dead_product, dead_proposal;  // [stage][descriptor]
};
static nbp_liveness product_liveness(const nbp_program *p) {
  nbp_liveness L;
  L.dead_product.resize(p->n_user_stages);
  L.dead_proposal.resize(p->n_user_stages);
  struct Open { int stage, idx, pstage, pidx; };  // pstage >= 0: pass-through of that proposal's KDE
  std::unordered_map<int32_t, Open> open;                        // slot -> unresolved product output
  std::unordered_map<int32_t, std::pair<int, int>> last_prop;    // scratch slot -> proposal that wrote it
  // proposals whose own KDE (points + bandwidth) is read directly: an input of a real product, the message of a
  // MsgPrior, a measurement KDE or the source of a slot copy.  Such a fit is live whatever happens to the output of
  // a pass-through product that also carries it.
  std::vector<std::pair<int, int>> needed;
  auto read_kde = [&](int32_t slot) {
    open.erase(slot);
    auto lp = last_prop.find(slot);
    if (lp != last_prop.end()) needed.push_back(lp->second);
  };
  auto kill = [&](int32_t slot) {
    auto it = open.find(slot);
    if (it == open.end()) return;
    const Open &o = it->second;
    if (o.pstage >= 0) L.dead_proposal[o.pstage][o.pidx] = 1;  // a pass-through hands on the proposal's own fit
    else L.dead_product[o.stage][o.idx] = 1;
    open.erase(it);
  };
  for (int s = 0; s < p->n_user_stages; s++) {
    const nbp_stage &st = p->stages[s];
    if (st.kind == NBP_STAGE_PROPOSALS) L.dead_proposal[s].assign(st.n, 0);
    if (st.kind == NBP_STAGE_PRODUCTS) L.dead_product[s].assign(st.n, 0);
    if (!p->lazy_bw) continue;  // every fit is made: nothing is dead
    if (st.kind == NBP_STAGE_COPIES && st.n == 0) {  // barrier: all live
      open.clear();
      for (auto &lp : last_prop) needed.push_back(lp.second);
    }
    // (a deconvolution counts as reading points only -- its outputs are always fitted; the measurement KDE it may name is
    //  not seen here: DESIGN.md 3)
    if (st.kind != NBP_STAGE_DECONV)
      stage_reads(p, st, [&](int, int32_t slot, nbp_access a) {
        if (a == NBP_RD_KDE) read_kde(slot);  // read: live
        else if (a == NBP_RD_CARRY) open.erase(slot);  // pass-through: the proposal's fit travels with the output (below)
      });
    stage_writes(p, st, [&](int i, int32_t slot) {
      kill(slot);  // overwritten
      if (st.kind == NBP_STAGE_PROPOSALS) { last_prop[slot] = {s, i}; return; }
      if (st.kind == NBP_STAGE_PRODUCTS) {
        const nbp_product_desc &q = ((const nbp_product_desc *)(p->blob.data() + st.offset))[i];
        if (q.nfactors > 1) {
          open[slot] = {s, i, -1, -1};
        } else {  // pass-through: the output carries the bandwidth fitted for the proposal
          auto lp = last_prop.find(q.in_slot[0]);
          if (lp != last_prop.end() && !((const nbp_proposal_desc *)(p->blob.data() + p->stages[lp->second.first].offset))[lp->second.second].skip_bandwidth)
            open[slot] = {s, i, lp->second.first, lp->second.second};
        }
      }
      last_prop.erase(slot);
    });
  }
  for (auto &nd : needed) L.dead_proposal[nd.first][nd.second] = 0;
  return L;  // whatever is still open is flushed at the end of the program: live
}

// ---- fused variable updates ---------------------------------------------------------------------------------------------
// A PROPOSALS stage followed by the PRODUCTS stage that multiplies exactly its proposals -- one round of Gibbs steps, as
// both hosts emit it -- runs as one launch of the fused update kernel when the round fills the chip and is of a class the
// kernel is built for.  What must hold (checked here, so that any program a caller assembles stays correct):
//   * every input of every product is the output of exactly one proposal of the stage in front, and every proposal feeds
//     exactly one product (the proposals never reach HBM; one that a later stage reads from its slot is written there too);
//   * no proposal reads a slot another update of the round writes (the three-launch form runs all proposals before any
//     product; fused, the updates of a round run in any order) -- rounds of commuting Gibbs steps satisfy this by construction;
//   * class (proposals_uniform_class = NBP_CLS_LIN2, simple or not): Euclid(2) throughout; full (non-partial) LinearRelative,
//     Prior, MsgPrior and pass-through proposals, with nullhypo, multihypo (nvars > 2), mixtures, injected / recorded
//     hypothesis indices, stored measurements (meas_seed), a KDE as the measurement (meas_kde), either solve direction,
//     operands of fewer than N points; 1 .. NBP_FUSED_MAXF inputs per product; skip_bandwidth only on the lone proposal of
//     a pass-through product; a pass-through among several inputs, or alone with keep_count = 0;
//   * refused: another manifold, partial proposals, relatives of another kind; products with label output, an old_slot
//     (hence partial inputs), more than NBP_FUSED_MAXF inputs; Npad > 256; an LDS need above 158 KiB (nbp_program_finalize).
//   The same bits as the three-launch form either way (tests/fused_cases.py keeps one round per entry of both lists).
static bool fused_plan(const nbp_program *p, int s, std::vector<nbp_update_desc> &upd, int &Fmax) {
  const nbp_ctx *c = p->ctx;
  if (!c->fused_on || !p->use_fused || s + 1 >= p->n_user_stages || c->Npad > 256) return false;
  const nbp_stage &A = p->stages[s], &B = p->stages[s + 1];
  if (A.kind != NBP_STAGE_PROPOSALS || B.kind != NBP_STAGE_PRODUCTS || B.n < c->fused_min || A.n < B.n) return false;
  if ((A.mani & (NBP_CLS_SIMPLE - 1)) != NBP_CLS_LIN2) return false;
  const int M = NBP_EUCLID2;
  const nbp_proposal_desc *pd = (const nbp_proposal_desc *)(p->blob.data() + A.offset);
  const nbp_product_desc *qd = (const nbp_product_desc *)(p->blob.data() + B.offset);
  std::unordered_map<int32_t, int> prop_of, prod_of;  // slot -> proposal / product writing it
  for (int i = 0; i < A.n; i++) {
    if (pd[i].manifold != M) return false;
    if (!prop_of.emplace(pd[i].out_slot, i).second) return false;
  }
  for (int i = 0; i < B.n; i++) {
    if (qd[i].manifold != M || qd[i].nfactors > NBP_FUSED_MAXF || qd[i].labels_out >= 0 || qd[i].old_slot >= 0) return false;
    if (!prod_of.emplace(qd[i].out_slot, i).second) return false;
  }
  upd.assign(B.n, nbp_update_desc{});
  std::vector<char> used(A.n, 0);
  int nused = 0;
  Fmax = 2;
  for (int i = 0; i < B.n; i++) {
    nbp_update_desc &u = upd[i];
    u.prod = i;
    if (qd[i].nfactors > Fmax) Fmax = qd[i].nfactors;
    for (int j = 0; j < qd[i].nfactors; j++) {
      if (qd[i].in_partial[j]) return false;
      auto it = prop_of.find(qd[i].in_slot[j]);
      if (it == prop_of.end() || used[it->second]) return false;
      const nbp_proposal_desc &q = pd[it->second];
      if (qd[i].nfactors > 1 && q.skip_bandwidth && q.factor_kind != NBP_F_PASSTHROUGH) return false;  // the product would read a stale bandwidth
      if (q.factor_kind == NBP_F_PASSTHROUGH && qd[i].nfactors == 1 && q.keep_count) return false;
      used[it->second] = 1;
      nused++;
      u.prop[j] = it->second;
      // what the proposal reads: never a slot that another update of this launch writes, nor another proposal's slot
      bool clash = false;
      proposal_reads(q, [&](int32_t r, nbp_access) {
        auto w = prod_of.find(r);
        clash |= (w != prod_of.end() && w->second != i) || prop_of.count(r);
      });
      if (clash) return false;
    }
  }
  if (nused != A.n) return false;
  // proposals a later stage reads from their arena slots before anything overwrites them (or that are still there when the
  // program ends): those are written as well
  std::unordered_map<int32_t, std::pair<int, int>> watch;  // slot -> (update, input)
  for (int i = 0; i < B.n; i++)
    for (int j = 0; j < qd[i].nfactors; j++) watch[qd[i].in_slot[j]] = {i, j};
  for (int i = 0; i < B.n; i++) watch.erase(qd[i].out_slot);  // (a product writing a proposal slot: overwritten at once)
  for (int t = s + 2; t < p->n_user_stages && !watch.empty(); t++) {
    const nbp_stage &st = p->stages[t];
    // barrier: slots leave the device -- whatever is still watched is written (below)
    if ((st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS) && st.n == 0) break;
    stage_reads(p, st, [&](int, int32_t slot, nbp_access) {
      auto it = watch.find(slot);
      if (it == watch.end()) return;
      upd[it->second.first].flags |= 2 << it->second.second;
      watch.erase(it);
    }, true);
    stage_writes(p, st, [&](int, int32_t slot) { watch.erase(slot); });
  }
  for (auto &w : watch) upd[w.second.first].flags |= 2 << w.second.second;
  return true;
}

static nbp_status launch_update(nbp_ctx *c, const nbp_stage &st, const nbp_update_desc *uds, const nbp_proposal_desc *props,
                                const nbp_product_desc *prods, int n) {
  nbp_status rc = tic(c, c->ev[4]);
  if (rc) return rc;
  (void)hipGetLastError();
  const int P = n >= c->fused_p1_min ? 1 : 2;
  const size_t lds = nbp_update_lds_bytes(st.upd_F, 2, c->N, c->Npad, P, false);
  hipLaunchKernelGGL(P == 1 ? nbp_update_kernel_lin2_p1 : nbp_update_kernel_lin2_p2, dim3(n), dim3(P * c->Npad), lds, c->stream, uds, props, prods,
                     c->arena, c->N, c->Npad, c->S, c->side, c->T, c->counters, st.upd_F);
  HIPCHK(hipGetLastError());
  return toc(c, c->ev[4]);
}

// ---- two-stream rounds --------------------------------------------------------------------------------------------------
// A round of many variable updates is three chip-filling launches with different bottlenecks: the proposal launch waits
// (barriers of the inflation cycles, divergent per-particle searches), the fit launch issues FP64 back to back, and every
// launch ends in a tail of partly filled CUs.  The updates of a round are independent of each other, so the round is cut
// in two halves that run the same three launches on two streams, the second half one launch behind the first:
//     stream 1:  proposals(a)  fits + KD(a)   products(a)                 join
//     stream 2:                proposals(b)   fits + KD(b)   products(b)
// What must hold for that to compute what the single-stream order computes: a product of half a must not write a slot a
// proposal of half b still has to read.  plan_pipeline() puts such updates into the same half (union-find over the
// products of the stage), balances the halves, and reorders the descriptors of both stages so that each half is a
// contiguous range.  Every launch of a half uses the geometry of the whole batch (helper rows per fit, lanes per sample),
// so no particle depends on the split: tests/test_gpu_pipelined_rounds.py compares every slot, bit for bit.
// ---- lanes --------------------------------------------------------------------------------------------------------------
// A tree pass batches round tt - start[c] of every running clique into stage tt, so a clique with a long schedule pays for
// each of its rounds the time of whatever chip-filling stage it rides in, and runs its last rounds alone on an idle chip.
// The host that compiled the stages knows which cliques those are and says so (nbp_program_set_lanes); here the stages keep
// their place and their descriptors, and below them the program runs two lanes: lane 0 on the library stream, lane 1 on
// the second stream with launches of its own size.  plan_lanes moves the lane-1 descriptors of a stage behind the others
// (moved_to: the seed table stays in the caller's order); plan_parts cuts the stages into parts, schedules the pending
// fits per lane and derives from the slots what a part waits for on the other lane; run_lanes launches the parts.
// ---- sinks --------------------------------------------------------------------------------------------------------------
// The up pass of a tree batches a clique's round into the stage of that round, also the products nothing reads before the
// down pass: above the leaves the frontal of every clique, beside the pass-throughs of its separators, which alone carry
// the chain up the tree.  With NBP_OPT_UP_PASS_SINKS those products and their proposals run in one or two later stages of
// the pass, as launches that fill the chip, and the chain's stages shrink to the pass-throughs (the rules: nbp_sinks.h).
// plan_sinks says which descriptor runs where (in the caller's order, before anything moves); plan_lanes puts the ones that
// leave behind the ones that stay; gather_sinks copies, for every stage that gains descriptors, its remaining lane-0
// descriptors and the gained ones into an array of their own behind the stages' descriptors.  The stages themselves stay
// whole: per-kernel timing, NBP_NO_LANES / NBP_NO_SINKS and ranges that cut a region run them as they always have.
static size_t lane_desc_bytes(int kind) {  // descriptors that may leave lane 0's part of their stage; 0: the kind stays whole
  return kind == NBP_STAGE_PROPOSALS ? sizeof(nbp_proposal_desc) : (kind == NBP_STAGE_PRODUCTS ? sizeof(nbp_product_desc) :
         (kind == NBP_STAGE_COPY_POINTS ? sizeof(nbp_copy_desc) : 0));
}
static void plan_sinks(nbp_program *p) {
  if (!p->sinks || p->ctx->no_lanes || p->ctx->no_sinks) return;
  const int ns = p->n_user_stages;
  std::vector<nbp_sink_stage> sk((size_t)ns);
  // the up pass: the first run of stages between whole-slot copy stages (or empty copy stages: barriers) that holds products
  int first = -1, last = -1;
  for (int s = 0, from = 0; s <= ns && first < 0; s++) {
    const bool edge = s == ns || p->stages[(size_t)s].kind == NBP_STAGE_COPIES || (p->stages[(size_t)s].kind == NBP_STAGE_COPY_POINTS && p->stages[(size_t)s].n == 0);
    if (!edge) continue;
    for (int t = from; t < s; t++)
      if (p->stages[(size_t)t].kind == NBP_STAGE_PRODUCTS) { first = from; last = s - 1; break; }
    from = s + 1;
  }
  if (first < 0) return;
  for (int s = 0; s < ns; s++) {
    const nbp_stage &st = p->stages[(size_t)s];
    nbp_sink_stage &g = sk[(size_t)s];
    g.kind = st.kind == NBP_STAGE_PROPOSALS ? NBP_SINK_PROPOSALS : (st.kind == NBP_STAGE_PRODUCTS ? NBP_SINK_PRODUCTS : NBP_SINK_OTHER);
    g.pass = s >= first && s <= last ? 0 : -1;
    g.d.resize((size_t)st.n);
    for (int i = 0; i < st.n; i++) {
      g.d[(size_t)i].lane = !st.lane_hint.empty() && lane_desc_bytes(st.kind) ? st.lane_hint[(size_t)i] : 0;
      if (st.kind == NBP_STAGE_PRODUCTS) g.d[(size_t)i].nfactors = ((const nbp_product_desc *)(p->blob.data() + st.offset))[i].nfactors;
    }
    stage_touches(p, st, [&](int i, int32_t x) { g.d[(size_t)i].reads.push_back(x); }, [&](int i, int32_t x) { g.d[(size_t)i].writes.push_back(x); });
  }
  nbp_sink_plan(sk, p->ctx->sink_placement == 1 ? NBP_SINK_LAST : NBP_SINK_TWO);
  for (int s = 0; s < ns; s++) {
    nbp_stage &st = p->stages[(size_t)s];
    bool leaves = false;
    for (const nbp_sink_desc &d : sk[(size_t)s].d) leaves = leaves || d.to != s;
    if (!leaves) continue;
    st.sink_to.resize((size_t)st.n);
    for (int i = 0; i < st.n; i++) st.sink_to[(size_t)i] = sk[(size_t)s].d[(size_t)i].to;
    st.sink_touched = true;
    p->sunk = true;
  }
}

static void plan_lanes(nbp_program *p) {
  if (p->ctx->no_lanes) return;
  for (int s = 0; s < p->n_user_stages; s++) {
    nbp_stage &st = p->stages[(size_t)s];
    if (st.lane_hint.empty() && st.sink_to.empty()) continue;
    const size_t esz = lane_desc_bytes(st.kind);
    if (!esz) continue;  // whole-slot copies and deconvolutions stay on lane 0
    // lane 0's descriptors that stay, lane 0's that leave for a sink (they are lane 0's: nbp_sinks.h), lane 1's
    auto place = [&](int i) { return !st.lane_hint.empty() && st.lane_hint[(size_t)i] ? 2 : (!st.sink_to.empty() && st.sink_to[(size_t)i] != s ? 1 : 0); };
    int cnt[3] = {0, 0, 0};
    for (int i = 0; i < st.n; i++) cnt[place(i)]++;
    if (!cnt[1] && !cnt[2]) continue;
    std::vector<char> moved((size_t)st.n * esz);
    st.moved_to.assign((size_t)st.n, 0);
    int at = 0;
    for (int l = 0; l < 3; l++)
      for (int i = 0; i < st.n; i++)
        if (place(i) == l) {
          st.moved_to[(size_t)i] = at;
          memcpy(moved.data() + (size_t)at++ * esz, p->blob.data() + st.offset + (size_t)i * esz, esz);
        }
    memcpy(p->blob.data() + st.offset, moved.data(), moved.size());
    if (cnt[2]) st.lane_split = st.n - cnt[2];
    if (cnt[1]) st.sink_stay = cnt[0];
  }
}

// the gathered copies (behind the descriptors of the stages, in front of everything layout_blob appends), and per sink the
// stages its updates span
static void gather_sinks(nbp_program *p) {
  if (!p->sunk) return;
  const int ns = p->n_user_stages;
  std::vector<std::vector<std::pair<int, int>>> came((size_t)ns);  // per stage: (stage, place there now) of what it gains, in list order
  std::vector<int> from((size_t)ns, -1);
  for (int s = 0; s < ns; s++) {
    const nbp_stage &st = p->stages[(size_t)s];
    for (int i = 0; i < (int)st.sink_to.size(); i++) {
      const int to = st.sink_to[(size_t)i];
      if (to == s) continue;
      came[(size_t)to].push_back({s, st.moved_to[(size_t)i]});
      if (from[(size_t)to] < 0) from[(size_t)to] = s;
    }
  }
  for (int s = 0; s < ns; s++) {
    if (came[(size_t)s].empty()) continue;
    nbp_stage &st = p->stages[(size_t)s];
    const size_t esz = lane_desc_bytes(st.kind);
    const int own = st.sink_stay >= 0 ? st.sink_stay : (st.lane_split >= 0 ? st.lane_split : st.n);
    for (int i = 0; i < own; i++) st.gather_src.push_back({s, i});
    for (auto &c : came[(size_t)s]) st.gather_src.push_back(c);
    st.gained = (int)came[(size_t)s].size();
    st.gather_n = (int)st.gather_src.size();
    st.gather_off = (p->blob.size() + 63) & ~(size_t)63;
    st.sink_touched = true;
    p->blob.resize(st.gather_off + (size_t)st.gather_n * esz);
    for (int j = 0; j < st.gather_n; j++)
      memcpy(p->blob.data() + st.gather_off + (size_t)j * esz,
             p->blob.data() + p->stages[(size_t)st.gather_src[(size_t)j].first].offset + (size_t)st.gather_src[(size_t)j].second * esz, esz);
    // (from the proposal stage in front of the first product that left to the sink's product stage)
    if (st.kind == NBP_STAGE_PRODUCTS) p->sink_regions.push_back({from[(size_t)s] - 1, s});
  }
}

static void plan_pipeline(nbp_program *p, int s) {
  nbp_stage &ps = p->stages[s], &qs = p->stages[s + 1];
  if (ps.kind != NBP_STAGE_PROPOSALS || qs.kind != NBP_STAGE_PRODUCTS || qs.n < p->ctx->pipe_min || qs.n < 128) return;
  if (ps.lane_split >= 0 || qs.lane_split >= 0) return;  // lanes win: a round with lane-1 descriptors is not cut in two as well
  if (ps.sink_touched || qs.sink_touched) return;        // nor one that updates leave or come to (the gathered copies are made)
  nbp_proposal_desc *pd = (nbp_proposal_desc *)(p->blob.data() + ps.offset);
  nbp_product_desc *qd = (nbp_product_desc *)(p->blob.data() + qs.offset);
  std::unordered_map<int32_t, int> prop_of, prod_of, reader_of;
  for (int i = 0; i < ps.n; i++) prop_of[pd[i].out_slot] = i;
  for (int i = 0; i < qs.n; i++) prod_of[qd[i].out_slot] = i;
  std::vector<int> uf(qs.n), owner(ps.n, -1);
  for (int i = 0; i < qs.n; i++) uf[i] = i;
  auto find = [&](int a) { while (uf[a] != a) a = uf[a] = uf[uf[a]]; return a; };
  auto unite = [&](int a, int b) { a = find(a); b = find(b); if (a != b) uf[a] = b; };
  for (int i = 0; i < qs.n; i++) {
    if (qd[i].old_slot >= 0) return;  // partial products top their old points up inside the fit launch: left alone
    for (int j = 0; j < qd[i].nfactors; j++) {
      // two products reading one density (a proposal, or a message whose fit is still pending) stay together: the fit of
      // that density runs in one half only
      auto rd = reader_of.find(qd[i].in_slot[j]);
      if (rd == reader_of.end()) reader_of[qd[i].in_slot[j]] = i; else unite(rd->second, i);
      auto it = prop_of.find(qd[i].in_slot[j]);
      if (it != prop_of.end() && owner[it->second] < 0) owner[it->second] = i;
    }
  }
  stage_reads(p, ps, [&](int k, int32_t slot, nbp_access) {
    if (owner[k] < 0) return;  // feeds no product of this round: first half, done before any product starts
    auto it = prod_of.find(slot);
    if (it != prod_of.end()) unite(owner[k], it->second);
  });
  // components, largest first, each to the lighter half (weight: densities, the unit of the fit and KD work)
  std::unordered_map<int, std::pair<int, std::vector<int>>> comp;
  for (int i = 0; i < qs.n; i++) { auto &c = comp[find(i)]; c.first += qd[i].nfactors; c.second.push_back(i); }
  std::vector<std::pair<int, std::vector<int>>> cs;
  for (auto &kv : comp) cs.push_back(std::move(kv.second));
  std::sort(cs.begin(), cs.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second[0] < b.second[0]; });
  std::vector<char> half(qs.n, 0);
  int w[2] = {0, 0}, cnt[2] = {0, 0};
  for (auto &c : cs) {
    const int h = w[1] < w[0] ? 1 : 0;
    w[h] += c.first;
    for (int i : c.second) { half[i] = (char)h; cnt[h]++; }
  }
  if (cnt[0] < qs.n / 3 || cnt[1] < qs.n / 3) return;  // one big component: nothing to run side by side
  std::vector<nbp_product_desc> q2;
  qs.moved_to.assign((size_t)qs.n, 0);
  for (int h = 0; h < 2; h++)
    for (int i = 0; i < qs.n; i++) if (half[i] == h) { qs.moved_to[(size_t)i] = (int)q2.size(); q2.push_back(qd[i]); }
  std::vector<nbp_proposal_desc> p2;
  ps.moved_to.assign((size_t)ps.n, 0);
  int np0 = 0;
  for (int h = 0; h < 2; h++)
    for (int k = 0; k < ps.n; k++) {
      const int hk = owner[k] < 0 ? 0 : half[owner[k]];
      if (hk == h) { ps.moved_to[(size_t)k] = (int)p2.size(); p2.push_back(pd[k]); np0 += h == 0; }
    }
  memcpy(qd, q2.data(), q2.size() * sizeof(nbp_product_desc));
  memcpy(pd, p2.data(), p2.size() * sizeof(nbp_proposal_desc));
  ps.pipe_split = np0;
  qs.pipe_split = cnt[0];
}

// The round at stages s, s + 1 runs as one launch of the fused update kernel (fused_plan agreed): every fit of the round
// happens inside the launch -- what is pending runs first, nothing is queued behind it.  The PRODUCTS stage keeps the lists
// of a range that splits the pair (never read when the pair runs as one launch).
static void schedule_fused_pair(nbp_program *p, int s, std::vector<nbp_update_desc> &upd, int Fmax, const nbp_liveness &live, nbp_fits &pend) {
  nbp_stage &st = p->stages[s], &nx = p->stages[s + 1];
  const nbp_proposal_desc *pd = (const nbp_proposal_desc *)(p->blob.data() + st.offset);
  const nbp_product_desc *qd = (const nbp_product_desc *)(p->blob.data() + nx.offset);
  nx.split_out.clear();
  for (int i = 0; i < nx.n; i++) {
    // the output's fit: a real product's own, or the one a pass-through hands on from its proposal
    const int k = upd[i].prop[0];
    if (wants_fit(qd[i]) ? live.dead_product[s + 1][i] : (!wants_fit(pd[k]) || live.dead_proposal[s][k])) continue;
    upd[i].flags |= NBP_UPD_FIT_OUT;
    nx.split_out.push(qd[i].out_slot, qd[i].manifold);
  }
  nx.ent.clear();
  queue_fits(nx.ent, pd, st.n);  // (of every proposal, dead or not, as the three-launch form of a split range has always made them)
  nx.fused_second = true;
  nx.need_prep = false;
  st.fused = true;
  st.upd = std::move(upd);
  st.upd_F = Fmax;
  st.flush_before = !pend.empty();
  pend.clear();
}

// The walk over the pending fits: what each stage finds queued at its entry (`ent`), whether that must run before it
// (`flush_before`), and what it queues in turn.
static void schedule_fits(nbp_program *p, const nbp_liveness &live) {
  nbp_fits pend;
  for (int s = 0; s < (int)p->stages.size(); s++) {
    nbp_stage &st = p->stages[s];
    if (st.fused_second) continue;  // ran inside the launch of the stage in front (schedule_fused_pair)
    const char *d = p->blob.data() + st.offset;
    st.ent = pend;
    auto flush_if_read = [&](nbp_access what) {  // a fit still pending for a slot the stage reads that way runs first
      stage_reads(p, st, [&](int, int32_t slot, nbp_access a) { st.flush_before |= a == what && pend.has(slot); });
      if (st.flush_before) pend.clear();
    };
    if (st.kind == NBP_STAGE_PROPOSALS) {
      std::vector<nbp_update_desc> upd;
      int Fm = 0;
      if (s + 1 < p->n_user_stages && fused_plan(p, s, upd, Fm) && nbp_update_lds_bytes(Fm, 2, p->ctx->N, p->ctx->Npad, 2, false) <= 158 * 1024) {
        schedule_fused_pair(p, s, upd, Fm, live, pend);
        continue;
      }
      flush_if_read(NBP_RD_KDE);  // a MsgPrior samples from the KDE in var_slot[1], a measurement KDE: points AND bandwidth
      queue_fits(pend, (const nbp_proposal_desc *)d, st.n, live.dead_proposal[s].data());
    } else if (st.kind == NBP_STAGE_PRODUCTS) {
      const nbp_product_desc *qd = (const nbp_product_desc *)d;
      st.need_prep = false;
      for (int i = 0; i < st.n; i++) st.need_prep |= qd[i].nfactors > 1;
      // the prep launch tops up the oldPoints of a partial product in place (topup_slot: reads the slot's bandwidth and
      // count, writes points and count) beside the fits of the same launch: a fit still pending for that very slot would
      // race with it, so such fits run first, in a launch of their own  (old_slot is the one points-only read of a product)
      flush_if_read(NBP_RD_POINTS);
      if (st.need_prep) {
        pend.clear();  // the entry fits run inside this stage's prep launch
      } else {
        // Only pass-through products (AMP returns the single density): nothing here reads a bandwidth, so nothing is
        // launched for the fits.  A pending fit of a density that is handed on moves with it -- same points, same
        // bandwidth, fitted in the output slot when the next launch with fits comes along (graph initialisation of a
        // chain: one proposal + one copy per variable on the critical path, all the fits in one launch at the end).
        for (int i = 0; i < st.n; i++) pend.rename(qd[i].in_slot[0], qd[i].out_slot);
        // (an output slot whose OLD points still had a fit queued: that fit would now see the new points -- which is what
        //  the reference's setBelief! does anyway: manikde! of the points it stores)
        pend.dedup();
      }
      queue_fits(pend, qd, st.n, live.dead_product[s].data());
    } else if (st.kind == NBP_STAGE_DECONV || st.kind == NBP_STAGE_COPY_POINTS) {
      // nothing is flushed (points only are read); a fit still queued for a slot that is overwritten would see the new
      // points: void.  A deconvolution queues the fits of its outputs.
      stage_writes(p, st, [&](int, int32_t slot) { pend.drop(slot); });
      st.ent = pend;
      if (st.kind == NBP_STAGE_DECONV)
        for (int i = 0; i < st.n; i++) pend.push(((const nbp_proposal_desc *)d)[i].out_slot, ((const nbp_proposal_desc *)d)[i].manifold);
    } else {  // copies (move bandwidths too) and the trailing pseudo stage
      st.flush_before = true;
      pend.clear();
    }
  }
}

// A round that plan_pipeline cut in two runs on two streams unless it is fused, has no prep launch, flushes first, or has
// products too large for the LDS (they share one node-statistics workspace: the launch's own decision).  Its entry fits
// are reordered like its descriptors: those of densities only the first half's products read, then the rest.
static void split_piped_entry_fits(nbp_program *p) {
  for (int s = 0; s + 1 < p->n_user_stages; s++) {
    nbp_stage &ps = p->stages[s], &qs = p->stages[s + 1];
    if (ps.kind != NBP_STAGE_PROPOSALS || qs.kind != NBP_STAGE_PRODUCTS || ps.pipe_split < 0 || qs.pipe_split < 0) continue;
    if (ps.fused || !qs.need_prep || qs.flush_before) continue;
    nbp_launch_env round = ctx_env(p->ctx);
    round.geom_n = qs.n;
    if (product_plan(p->ctx, round, qs.n, qs.maxfd, qs.mani).big) continue;
    const nbp_product_desc *qd = (const nbp_product_desc *)(p->blob.data() + qs.offset);
    std::unordered_map<int32_t, int> second;  // slots the second half's products read
    for (int i = qs.pipe_split; i < qs.n; i++)
      for (int j = 0; j < qd[i].nfactors; j++) second[qd[i].in_slot[j]] = 1;
    nbp_fits ent;
    for (int h = 0; h < 2; h++)
      for (const nbp_fits::fit &f : qs.ent.v)
        if ((int)second.count(f.slot) == h) { ent.push(f.slot, f.mani); if (!h) qs.pipe_ent++; }
    qs.ent = ent;
    ps.pipe = true;
  }
}

// The parts of a program with lanes, their fits and their waits.  The stages themselves keep the schedule schedule_fits gave
// them: a run without lanes (timing, a range that cuts a lane-1 region) launches them whole, as it always has.
//   * parts: per stage its lane-0 descriptors, then its lane-1 descriptors; a trailing pseudo part like the trailing stage.
//   * fits: one pending list per lane, walked like schedule_fits walks the one list.  A part that needs the bandwidth of a
//     slot whose fit is pending on the OTHER lane, or overwrites such a slot, takes the fit over: it runs on the lane of
//     the part that first reads its result (a points-only read leaves it where it is: a fit does not touch the points).  A
//     points-only overwrite voids a pending fit on either lane.  Whole-slot copies and the end of the program take over
//     everything.
//   * waits: nbp_lane_sweep over what every part reads and writes, its fits included -- the points and the bandwidth of a
//     slot apart (2 * slot, 2 * slot + 1): a fit reads the points and writes the bandwidth; the side buffer (hypothesis
//     indices, labels) counts as one slot, an empty copy stage is a barrier.
// No lanes (parts stay empty) where a stage with lane-1 descriptors runs fused.
// Sinks (plan_sinks, gather_sinks): the lane-0 part of a stage that updates left is the descriptors that stay; the lane-0 part
// of a sink stage is the gathered copy.  Everything below walks the parts as they will run, so the fits, the liveness rows,
// the workspaces and the waits follow the moved list by themselves.  No sinks where a stage they touch runs fused.
static void plan_parts(nbp_program *p, const nbp_liveness &live) {
  bool any = false;
  for (int s = 0; s < p->n_user_stages; s++) {
    const nbp_stage &st = p->stages[(size_t)s];
    if (st.lane_split < 0) continue;
    if (st.fused || st.fused_second) return;
    any = true;
  }
  for (int s = 0; s < p->n_user_stages && p->sunk; s++)
    if (p->stages[(size_t)s].sink_touched && (p->stages[(size_t)s].fused || p->stages[(size_t)s].fused_second)) p->sunk = false;
  if (!any && !p->sunk) return;
  std::vector<nbp_stage> &parts = p->parts;
  std::vector<const char *> dead;  // per part: the liveness row of its descriptors
  std::vector<std::vector<char>> dead_gathered((size_t)p->n_user_stages);  // (of a gathered part: gathered like its descriptors)
  auto dead_row = [&](int s) -> const std::vector<char> & {
    return p->stages[(size_t)s].kind == NBP_STAGE_PRODUCTS ? live.dead_product[(size_t)s] : live.dead_proposal[(size_t)s];
  };
  p->first_part.assign((size_t)p->n_user_stages + 1, 0);
  for (int s = 0; s < p->n_user_stages; s++) {
    const nbp_stage &st = p->stages[(size_t)s];
    p->first_part[(size_t)s] = (int)parts.size();
    const size_t esz = st.kind == NBP_STAGE_PRODUCTS ? sizeof(nbp_product_desc) : (st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS ?
                       sizeof(nbp_copy_desc) : sizeof(nbp_proposal_desc));
    const int cut = st.lane_split < 0 ? st.n : st.lane_split;
    for (int l = 0; l < 2; l++) {
      const bool gathered = !l && p->sunk && st.gather_n > 0;
      const int from = l ? cut : 0, n = l ? st.n - cut : (gathered ? st.gather_n : (p->sunk && st.sink_stay >= 0 ? st.sink_stay : cut));
      if (n == 0 && (l || st.lane_split >= 0 || st.n > 0)) continue;  // (an empty stage stays, as one empty lane-0 part: the barrier)
      nbp_stage pt;
      pt.kind = st.kind; pt.n = n; pt.offset = gathered ? st.gather_off : st.offset + (size_t)from * esz; pt.lane = l; pt.user = s;
      pt.maxfd = st.maxfd; pt.mani = st.mani;
      pt.gathered = gathered;
      pt.gained = gathered ? st.gained : 0;
      if (st.kind == NBP_STAGE_PRODUCTS && (n != st.n || gathered)) {
        pt.maxfd = products_maxfd((const nbp_product_desc *)(p->blob.data() + pt.offset), n);
        pt.mani = products_uniform_manifold((const nbp_product_desc *)(p->blob.data() + pt.offset), n);
      }
      if (st.kind == NBP_STAGE_PROPOSALS && (n != st.n || gathered)) pt.mani = proposals_uniform_class((const nbp_proposal_desc *)(p->blob.data() + pt.offset), n);
      const std::vector<char> &row = dead_row(s);
      if (gathered && (st.kind == NBP_STAGE_PRODUCTS || st.kind == NBP_STAGE_PROPOSALS)) {
        std::vector<char> &g = dead_gathered[(size_t)s];
        for (const auto &src : st.gather_src) g.push_back(dead_row(src.first)[(size_t)src.second]);
        dead.push_back(g.data());
      } else {
        dead.push_back(row.empty() ? nullptr : row.data() + from);
      }
      parts.push_back(std::move(pt));
    }
  }
  p->first_part[(size_t)p->n_user_stages] = (int)parts.size();
  {
    nbp_stage pt;  // trailing pseudo part (kind 0)
    pt.user = p->n_user_stages;
    dead.push_back(nullptr);
    parts.push_back(std::move(pt));
  }
  // ---- the pending fits, per lane
  nbp_fits pend[2];
  std::vector<nbp_fits> ran(parts.size());  // what each part runs of fits, for the sweep
  for (int k = 0; k < (int)parts.size(); k++) {
    nbp_stage &st = parts[(size_t)k];
    const int l = st.lane, o = 1 - l;
    const char *d = p->blob.data() + st.offset;
    if (k == p->first_part[(size_t)st.user]) {
      st.bound = pend[0];
      for (const nbp_fits::fit &f : pend[1].v) st.bound.push(f.slot, f.mani);
    }
    if (st.kind == NBP_STAGE_DECONV || st.kind == NBP_STAGE_COPY_POINTS)  // points-only overwrite: the fit of the old points is void
      stage_writes(p, st, [&](int, int32_t slot) { pend[0].drop(slot); pend[1].drop(slot); });
    if (!pend[o].empty()) {  // fits pending on the other lane that this part needs, or whose slots it overwrites: taken over
      auto claim = [&](int32_t slot) {
        for (size_t i = 0; i < pend[o].v.size();)
          if (pend[o].v[i].slot == slot) { pend[l].v.push_back(pend[o].v[i]); pend[o].v.erase(pend[o].v.begin() + (long)i); } else i++;
      };
      // (the one points-only read of a product is its old_slot, topped up in place from the slot's bandwidth: schedule_fits)
      stage_reads(p, st, [&](int, int32_t slot, nbp_access a) { if (a != NBP_RD_POINTS || st.kind == NBP_STAGE_PRODUCTS) claim(slot); });
      if (st.kind == NBP_STAGE_PROPOSALS || st.kind == NBP_STAGE_PRODUCTS) stage_writes(p, st, [&](int, int32_t slot) { claim(slot); });
      if (st.kind == NBP_STAGE_COPIES || st.kind == 0) {
        for (const nbp_fits::fit &f : pend[o].v) pend[l].v.push_back(f);
        pend[o].clear();
      }
    }
    st.ent = pend[l];
    auto flush_if_read = [&](nbp_access what) {
      stage_reads(p, st, [&](int, int32_t slot, nbp_access a) { st.flush_before |= a == what && pend[l].has(slot); });
      if (st.flush_before) { for (const nbp_fits::fit &f : pend[l].v) ran[(size_t)k].push(f.slot, f.mani); pend[l].clear(); }
    };
    if (st.kind == NBP_STAGE_PROPOSALS) {
      flush_if_read(NBP_RD_KDE);
      queue_fits(pend[l], (const nbp_proposal_desc *)d, st.n, dead[(size_t)k]);
    } else if (st.kind == NBP_STAGE_PRODUCTS) {
      const nbp_product_desc *qd = (const nbp_product_desc *)d;
      st.need_prep = false;
      for (int i = 0; i < st.n; i++) st.need_prep |= qd[i].nfactors > 1;
      flush_if_read(NBP_RD_POINTS);
      if (st.need_prep) {
        for (const nbp_fits::fit &f : pend[l].v) ran[(size_t)k].push(f.slot, f.mani);
        pend[l].clear();
      } else {
        for (int i = 0; i < st.n; i++) pend[l].rename(qd[i].in_slot[0], qd[i].out_slot);
        pend[l].dedup();
      }
      queue_fits(pend[l], qd, st.n, dead[(size_t)k]);
    } else if (st.kind == NBP_STAGE_DECONV || st.kind == NBP_STAGE_COPY_POINTS) {
      if (st.kind == NBP_STAGE_DECONV)
        for (int i = 0; i < st.n; i++) pend[l].push(((const nbp_proposal_desc *)d)[i].out_slot, ((const nbp_proposal_desc *)d)[i].manifold);
    } else {  // whole-slot copies and the trailing pseudo part: everything pending runs first
      st.flush_before = true;
      for (const nbp_fits::fit &f : pend[l].v) ran[(size_t)k].push(f.slot, f.mani);
      pend[l].clear();
    }
  }
  // ---- what a part waits for on the other lane
  std::vector<nbp_lane_part> sw(parts.size());
  for (int k = 0; k < (int)parts.size(); k++) {
    const nbp_stage &st = parts[(size_t)k];
    nbp_lane_part &a = sw[(size_t)k];
    a.stage = st.user;
    a.lane = st.lane;
    a.barrier = st.kind == 0 || ((st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS) && st.n == 0);
    stage_touches(p, st, [&](int, int32_t x) { a.reads.push_back(x); }, [&](int, int32_t x) { a.writes.push_back(x); });
    for (const nbp_fits::fit &f : ran[(size_t)k].v) { a.reads.push_back(2 * f.slot); a.writes.push_back(2 * f.slot + 1); }
  }
  nbp_lane_sweep(sw);
  for (int k = 0; k < (int)parts.size(); k++) {
    parts[(size_t)k].waits = sw[(size_t)k].waits;
    parts[(size_t)k].signals = sw[(size_t)k].signals;
  }
  // ---- what lane 1 needs of the workspaces (presize)
  for (const nbp_stage &st : parts)
    if (st.lane == 1 && st.kind == NBP_STAGE_PRODUCTS && st.n > 0) {
      p->lane_ws = std::max(p->lane_ws, (size_t)st.n * (size_t)(st.maxfd / 4) * nbp_kd_ws_doubles(p->ctx->N));
      nbp_launch_env env = ctx_env(p->ctx);
      p->lane_gstats = std::max(p->lane_gstats, std::max(product_plan(p->ctx, env, st.n, st.maxfd, st.mani).gstats, product_plan(p->ctx, env, st.n, st.maxfd, -1).gstats));
    }
}

// Behind the descriptors (and the gathered copies of the sinks, which gather_sinks has put right behind them), each region
// 64-byte aligned: the entry fits of every stage, the split-out fits of the fused pairs, the fits of the parts, the update
// descriptors, the seed table with the copies' entries, the seed values, the entries the copies follow.  (This order and these sizes are what captured graphs and the plan
// cache of nbp_host.cpp hold offsets into.)
// The seed table is in the CALLER's order -- the stages as nbp_program_add_stage took them -- whatever plan_pipeline did to
// the descriptors of a two-stream round since (nbp_stage::moved_to): entry i is the field seeds[i] of nbp_program_set_seeds
// belongs to.  Whether a proposal has a meas_seed entry is read off the descriptor at its new place.
static void layout_blob(nbp_program *p) {
  for (nbp_stage &st : p->stages) append_fits(p->blob, st.ent);
  for (nbp_stage &st : p->stages)
    if (st.fused_second) append_fits(p->blob, st.split_out, 4);
  for (nbp_stage &st : p->parts) {  // (none in a program without lanes)
    append_fits(p->blob, st.ent);
    append_fits(p->blob, st.bound);
  }
  for (nbp_stage &st : p->stages)
    if (st.fused) {
      st.upd_off = (p->blob.size() + 63) & ~(size_t)63;
      p->blob.resize(st.upd_off + st.upd.size() * sizeof(nbp_update_desc));
      memcpy(p->blob.data() + st.upd_off, st.upd.data(), st.upd.size() * sizeof(nbp_update_desc));
    }
  std::vector<int64_t> so;  // blob offsets of every descriptor's seed field
  for (int s = 0; s < p->n_user_stages; s++) {
    const nbp_stage &st = p->stages[s];
    if (st.kind == NBP_STAGE_PROPOSALS || st.kind == NBP_STAGE_DECONV)
      for (int i = 0; i < st.n; i++) {
        const size_t o = st.offset + (size_t)(st.moved_to.empty() ? i : st.moved_to[(size_t)i]) * sizeof(nbp_proposal_desc);
        so.push_back((int64_t)(o + offsetof(nbp_proposal_desc, seed)));
        // a reused measurement names another op's seed: re-keyed the same way, it keeps naming that op
        if (((const nbp_proposal_desc *)(p->blob.data() + o))->meas_seed) so.push_back((int64_t)(o + offsetof(nbp_proposal_desc, meas_seed)));
      }
    else if (st.kind == NBP_STAGE_PRODUCTS)
      for (int i = 0; i < st.n; i++)
        so.push_back((int64_t)(st.offset + (size_t)(st.moved_to.empty() ? i : st.moved_to[(size_t)i]) * sizeof(nbp_product_desc) + offsetof(nbp_product_desc, seed)));
  }
  // (nbp_program_seed_order: the rank of every entry's offset = its place in a walk over the descriptors as they lie now)
  std::vector<int64_t> sorted(so);
  std::sort(sorted.begin(), sorted.end());
  p->seed_rank.resize(so.size());
  for (size_t i = 0; i < so.size(); i++) p->seed_rank[i] = (int32_t)(std::lower_bound(sorted.begin(), sorted.end(), so[i]) - sorted.begin());
  // The gathered copies of a sink (gather_sinks) carry seed fields of their own: each follows the entry of the table its
  // original has, so that nbp_program_reseed re-keys both alike and nbp_program_set_seeds writes both.  Their offsets stand
  // behind the table's n_seeds entries, the entries they follow behind the values.
  std::vector<int64_t> dup;
  std::vector<int32_t> dup_src;
  if (p->sunk || !p->sink_regions.empty()) {
    std::unordered_map<int64_t, int32_t> entry;
    for (size_t i = 0; i < so.size(); i++) entry[so[i]] = (int32_t)i;
    for (int s = 0; s < p->n_user_stages; s++) {
      const nbp_stage &st = p->stages[(size_t)s];
      const size_t esz = st.kind == NBP_STAGE_PRODUCTS ? sizeof(nbp_product_desc) : sizeof(nbp_proposal_desc);
      for (int j = 0; j < st.gather_n; j++) {
        const int64_t from = (int64_t)(p->stages[(size_t)st.gather_src[(size_t)j].first].offset + (size_t)st.gather_src[(size_t)j].second * esz);
        const int64_t to = (int64_t)(st.gather_off + (size_t)j * esz);
        for (size_t field : {st.kind == NBP_STAGE_PRODUCTS ? offsetof(nbp_product_desc, seed) : offsetof(nbp_proposal_desc, seed),
                             st.kind == NBP_STAGE_PRODUCTS ? (size_t)0 : offsetof(nbp_proposal_desc, meas_seed)}) {
          auto it = field ? entry.find(from + (int64_t)field) : entry.end();
          if (it == entry.end()) continue;
          dup.push_back(to + (int64_t)field);
          dup_src.push_back(it->second);
        }
      }
    }
  }
  p->seed_off = (p->blob.size() + 63) & ~(size_t)63;
  p->n_seeds = (int)so.size();
  p->n_dup = (int)dup.size();
  p->seed_val_off = p->seed_off + (so.size() + dup.size()) * 8;
  p->dup_src_off = p->seed_val_off + so.size() * 8;
  p->blob.resize(p->dup_src_off + dup.size() * 4);
  if (!so.empty()) memcpy(p->blob.data() + p->seed_off, so.data(), so.size() * 8);
  if (!dup.empty()) {
    memcpy(p->blob.data() + p->seed_off + so.size() * 8, dup.data(), dup.size() * 8);
    memcpy(p->blob.data() + p->dup_src_off, dup_src.data(), dup.size() * 4);
  }
}

// size the workspaces now: nothing may allocate once a launch sequence is being captured
static nbp_status presize(nbp_program *p) {
  for (const nbp_stage &st : p->stages)
    if (st.kind == NBP_STAGE_PRODUCTS && st.n > 0 && !st.fused_second) {
      nbp_status rc = presize_products(p->ctx, st.n, st.maxfd, st.mani);
      if (rc) return rc;
    }
  if (p->parts.empty()) return NBP_OK;
  for (const nbp_stage &st : p->parts)  // (a sink's part may hold more products than any stage)
    if (st.gathered && st.kind == NBP_STAGE_PRODUCTS) {
      nbp_status rc = presize_products(p->ctx, st.n, st.maxfd, st.mani);
      if (rc) return rc;
    }
  // lanes: lane 1 builds its KD trees in the last lane_ws doubles of the workspace, beside whatever lane 0 builds in front of
  // them (its largest part is no larger than the largest stage, sized above), and keeps its node statistics in an area of
  // its own
  nbp_ctx *c = p->ctx;
  // one event per part that the other lane waits for: lane 1 is issued ahead of lane 0 (run_lanes), so a recorded event must
  // keep its meaning until the last wait for it is issued
  size_t nsig = 0;
  for (const nbp_stage &st : p->parts) nsig += st.signals ? 1 : 0;
  while (c->lane_ev.size() < nsig) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->lane_ev.push_back(e);
  }
  size_t main = 0;
  for (const nbp_stage &st : p->parts)
    if (st.lane == 0 && st.kind == NBP_STAGE_PRODUCTS) main = std::max(main, (size_t)st.n * (size_t)(st.maxfd / 4) * nbp_kd_ws_doubles(c->N));
  if (main + p->lane_ws > c->ws_doubles) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream2));
    if (c->ws) HIPCHK(hipFree(c->ws));
    c->ws = nullptr;
    c->ws_doubles = 0;
    c->ws_gen++;
    const size_t grown = main + p->lane_ws + (main + p->lane_ws) / 4;
    HIPCHK(hipMalloc(&c->ws, grown * 8));
    c->ws_doubles = grown;
  }
  if (p->lane_gstats > c->gstats1_doubles) {
    HIPCHK(hipStreamSynchronize(c->stream2));
    if (c->gstats1) HIPCHK(hipFree(c->gstats1));
    c->gstats1 = nullptr;
    c->ws_gen++;
    c->gstats1_doubles = p->lane_gstats + p->lane_gstats / 4;
    HIPCHK(hipMalloc(&c->gstats1, c->gstats1_doubles * 8));
  }
  return NBP_OK;
}

// device memory for the blob: one a destroyed program left behind, if one is large enough (the smallest such), or new
static nbp_status acquire_device_blob(nbp_program *p) {
  const size_t bytes = p->blob.size() ? p->blob.size() : 64;
  auto &bc = p->ctx->blob_cache;
  int best = -1;
  for (size_t i = 0; i < bc.size(); i++)
    if (bc[i].second >= bytes && (best < 0 || bc[i].second < bc[(size_t)best].second)) best = (int)i;
  if (best >= 0) {
    p->dev = bc[(size_t)best].first;
    p->dev_bytes = bc[(size_t)best].second;
    bc.erase(bc.begin() + best);
    return NBP_OK;
  }
  p->dev_bytes = bytes < 65536 ? 65536 : bytes;
  HIPCHK(hipMalloc(&p->dev, p->dev_bytes));
  return NBP_OK;
}

static nbp_status upload_blob(nbp_program *p) {
  if (p->blob.empty()) return NBP_OK;
  if (p->async_upload) {
    // stream-ordered: behind whatever still reads a blob taken over from a retired program, in front of this program's launches
    nbp_ctx::pin_buf *b = pin_acquire(p->ctx, p->blob.size());
    if (!b) return fail(NBP_ERR_HIP, "pinned staging buffer");
    memcpy(b->p, p->blob.data(), p->blob.size());
    const hipError_t e = hipMemcpyAsync(p->dev, b->p, p->blob.size(), hipMemcpyHostToDevice, p->ctx->stream);
    pin_release_behind_stream(p->ctx, b);
    if (e != hipSuccess) return fail(NBP_ERR_HIP, std::string("hipMemcpyAsync (descriptors): ") + hipGetErrorString(e));
    return NBP_OK;
  }
  // (a blob from the cache may come from a RETIRED program whose launches are still queued: the library stream does not
  //  wait for the legacy stream this copy runs on)
  if (!p->ctx->retired.empty()) HIPCHK(hipStreamSynchronize(p->ctx->stream));
  HIPCHK(hipMemcpy(p->dev, p->blob.data(), p->blob.size(), hipMemcpyHostToDevice));
  return NBP_OK;
}

nbp_status nbp_program_finalize(nbp_program *p) {
  if (!p) return fail(NBP_ERR_ARG, "null argument");
  PROG_ALIVE(p);
  if (p->finalized) return NBP_OK;
  HIPCHK(hipSetDevice(p->ctx->device));
  p->n_user_stages = (int)p->stages.size();
  p->stages.emplace_back();  // trailing pseudo stage (kind 0): the fits pending at exit
  plan_sinks(p);  // (NBP_OPT_UP_PASS_SINKS) which update runs where: over the stages as the caller gave them
  plan_lanes(p);  // reorder descriptors: before anything indexes them
  gather_sinks(p);
  for (int s = 0; s < p->n_user_stages; s++) {  // a gathered copy is held to what nbp_program_add_stage asks of a stage
    const nbp_stage &st = p->stages[(size_t)s];
    if (!st.gather_n) continue;
    const nbp_status rc = st.kind == NBP_STAGE_PRODUCTS ? check_products(p->ctx, (const nbp_product_desc *)(p->blob.data() + st.gather_off), st.gather_n)
                                                        : check_proposals(p->ctx, (const nbp_proposal_desc *)(p->blob.data() + st.gather_off), st.gather_n);
    if (rc) return rc;
  }
  for (int s = 0; s + 1 < p->n_user_stages; s++) plan_pipeline(p, s);
  const nbp_liveness live = product_liveness(p);
  schedule_fits(p, live);
  split_piped_entry_fits(p);
  plan_parts(p, live);
  layout_blob(p);
  nbp_status rc = presize(p);
  if (!rc) rc = acquire_device_blob(p);
  if (!rc) rc = upload_blob(p);
  if (rc) return rc;
  p->finalized = true;
  return NBP_OK;
}

// A range runs on two lanes when it holds lane-1 descriptors and neither starts nor ends inside a run of stages that have
// some (the fits pending at such a place are spread over both lanes); not under per-kernel timing, whose events are the
// library stream's.  Otherwise: the stages whole, in order, on the library stream (run_range below).
static bool lanes_apply(const nbp_program *p, int first, int last) {
  if (p->parts.empty() || p->ctx->timing || first >= last) return false;
  auto has1 = [&](int s) { return s >= 0 && s < p->n_user_stages && p->stages[(size_t)s].lane_split >= 0; };
  if ((has1(first - 1) && has1(first)) || (has1(last - 1) && has1(last))) return false;
  // sinks: a range that starts or ends between the first stage an update left and the stage it runs in would run it twice
  // or never; one that holds the region whole runs the parts
  bool sink = false;
  if (p->sunk)
    for (const auto &r : p->sink_regions) {
      auto inside = [&](int cut) { return r.first < cut && cut <= r.second; };
      if (inside(first) || inside(last)) return false;
      sink = sink || (first <= r.first && r.second < last);
    }
  if (sink) return true;
  for (int s = first; s < last; s++)
    if (has1(s)) return true;
  return false;
}
static nbp_status run_lanes(nbp_program *p, int first, int last) {
  nbp_ctx *c = p->ctx;
  if (p->lane_ws > c->ws_doubles) return fail(NBP_ERR_RANGE, "KD workspace smaller than lane 1's share (sized at nbp_program_finalize)");
  nbp_launch_env env[2] = {ctx_env(c), ctx_env(c)};
  env[0].lane = 1;
  env[0].ws_doubles = c->ws_doubles - p->lane_ws;
  env[1].lane = 2;
  env[1].stream = c->stream2;
  env[1].ws = c->ws + env[0].ws_doubles;
  env[1].ws_doubles = p->lane_ws;
  const int k0 = p->first_part[(size_t)first], k1 = p->first_part[(size_t)last];
  std::vector<hipEvent_t> ev((size_t)(k1 - k0), nullptr);
  size_t nev = 0;
  std::vector<char> issued((size_t)(k1 - k0), 0);
#define LANECHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(NBP_ERR_HIP, std::string("lanes: " #expr ": ") + hipGetErrorString(e_)); } while (0)
  // fork: lane 1 starts behind whatever the library stream holds in front of the range
  LANECHK(hipEventRecord(c->lane_fork, c->stream));
  LANECHK(hipStreamWaitEvent(c->stream2, c->lane_fork, 0));
  // Issue order: each lane's parts in list order, and lane 1 ahead of lane 0 as far as its waits allow (a wait points
  // backwards in list order, so when lane 1's next part waits for a part not yet issued, lane 0's next part waits for none).
  // The order of issue orders nothing on the device; it decides the order of the edges of a captured graph.  The runtime
  // keeps the first successor of a node on the node's own queue and deals the others out in turn over its few queues: were
  // the lane-0 part that waits for a lane-1 part captured before that part's own successor, a chain of lane-1 parts would
  // move to the next queue at every such part and, every fourth time, land behind lane 0 on the library stream's.
  int nx[2] = {k0, k0};
  auto seek = [&](int l) { while (nx[l] < k1 && p->parts[(size_t)nx[l]].lane != l) nx[l]++; };
  auto ready = [&](int k) {
    for (int w : p->parts[(size_t)k].waits)
      if (w >= k0 && !issued[(size_t)(w - k0)]) return false;
    return true;
  };
  for (;;) {
    seek(0);
    seek(1);
    if (nx[0] >= k1 && nx[1] >= k1) break;
    const int l = nx[1] < k1 && (ready(nx[1]) || nx[0] >= k1) ? 1 : 0;
    const int k = nx[l]++;
    issued[(size_t)(k - k0)] = 1;
    const nbp_stage &st = p->parts[(size_t)k];
    nbp_launch_env &e = env[st.lane];
    for (int w : st.waits)
      if (w >= k0) {  // (a part in front of the range has finished: the fork)
        LANECHK(hipStreamWaitEvent(e.stream, ev[(size_t)(w - k0)], 0));
        c->lane_waits++;
      }
    int launches = 0;
    nbp_status rc = NBP_OK;
    if (st.flush_before && st.ent.size()) { rc = launch_bandwidth(c, e, fits_dev(st.ent, p->dev)); launches++; }
    if (rc) return rc;
    if (st.kind == NBP_STAGE_PROPOSALS) {
      rc = launch_proposals(c, e, (const nbp_proposal_desc *)(p->dev + st.offset), st.n, st.mani);
      launches += st.n > 0;
    } else if (st.kind == NBP_STAGE_PRODUCTS) {
      const nbp_product_desc *dd = (const nbp_product_desc *)(p->dev + st.offset);
      if (st.need_prep) { rc = launch_prep(c, e, fits_dev(st.ent, p->dev), dd, st.n, st.maxfd, st.mani); launches++; }
      if (!rc) rc = launch_products(c, e, dd, st.n, st.maxfd, st.mani);
      launches += st.n > 0;
      if (st.lane) c->lane_side_updates += st.n;
    } else if (st.kind == NBP_STAGE_DECONV) {
      rc = launch_deconv(c, (const nbp_proposal_desc *)(p->dev + st.offset), nullptr, st.n);
    } else {
      rc = launch_copies(c, (const nbp_copy_desc *)(p->dev + st.offset), st.n, st.kind == NBP_STAGE_COPY_POINTS, e.stream);
      launches += st.n > 0;
    }
    if (rc) return rc;
    if (st.lane) c->lane_side_launches += launches;
    if (st.gained) {
      c->sink_launches += launches;
      if (st.kind == NBP_STAGE_PRODUCTS) c->sunk_updates += st.gained;
    }
    if (st.signals) {
      if (nev >= c->lane_ev.size()) return fail(NBP_ERR_RANGE, "lanes: fewer events than signalling parts (sized at nbp_program_finalize)");
      ev[(size_t)(k - k0)] = c->lane_ev[nev++];
      LANECHK(hipEventRecord(ev[(size_t)(k - k0)], e.stream));
    }
  }
  // join, then whatever either lane still has pending where the range ends
  LANECHK(hipEventRecord(c->lane_join, c->stream2));
  LANECHK(hipStreamWaitEvent(c->stream, c->lane_join, 0));
#undef LANECHK
  return launch_bandwidth(c, ctx_env(c), fits_dev(p->parts[(size_t)k1].bound, p->dev));
}

static nbp_status run_range(nbp_program *p, int first, int last) {
  if (lanes_apply(p, first, last)) return run_lanes(p, first, last);
  nbp_ctx *c = p->ctx;
  nbp_launch_env env = ctx_env(c);
  for (int s = first; s < last; s++) {
    const nbp_stage &st = p->stages[s];
    nbp_status rc = NBP_OK;
    if (st.flush_before) rc = launch_bandwidth(c, env, fits_dev(st.ent, p->dev));
    if (rc) return rc;
    if (st.kind == NBP_STAGE_PROPOSALS && st.fused && s + 1 >= last) {
      // the range ends between the two stages of a fused pair: the proposals alone, to their arena slots; their fits are the
      // entry list of the stage behind, which the end of the range runs (below)
      rc = launch_proposals(c, env, (const nbp_proposal_desc *)(p->dev + st.offset), st.n, st.mani);
    } else if (st.kind == NBP_STAGE_PROPOSALS && st.fused) {
      const nbp_stage &nx = p->stages[s + 1];
      rc = launch_update(c, st, (const nbp_update_desc *)(p->dev + st.upd_off), (const nbp_proposal_desc *)(p->dev + st.offset),
                         (const nbp_product_desc *)(p->dev + nx.offset), nx.n);
      s++;  // the products ran inside
    } else if (st.kind == NBP_STAGE_PROPOSALS && st.pipe && !c->timing && s + 1 < last) {
      // two-stream round (plan_pipeline): the second half runs one launch behind the first.  Both launch with the geometry
      // of the whole batch; the second on stream2, its KD builds in the workspace behind the first half's.
      const nbp_stage &nx = p->stages[s + 1];
      const nbp_proposal_desc *pd = (const nbp_proposal_desc *)(p->dev + st.offset);
      const nbp_product_desc *dd = (const nbp_product_desc *)(p->dev + nx.offset);
      const int ne = nx.ent.size(), ea = nx.pipe_ent, qa = nx.pipe_split, pa = st.pipe_split;
      const size_t wsa = (size_t)qa * (size_t)(nx.maxfd / 4) * nbp_kd_ws_doubles(c->N);
      nbp_launch_env h[2] = {env, env};
      h[0].geom_n = h[1].geom_n = nx.n;
      h[0].geom_blocks = h[1].geom_blocks = 2 * ne + 2 * nx.n;
      h[1].stream = c->stream2;
      h[1].ws = env.ws + wsa;
      h[1].ws_doubles = env.ws_doubles - wsa;
      auto half = [&](int k) -> nbp_status {
        const nbp_product_desc *dh = dd + (k ? qa : 0);
        const int nq = k ? nx.n - qa : qa;
        nbp_status r = launch_prep(c, h[k], fits_dev(nx.ent, p->dev, k ? ea : 0, k ? ne - ea : ea), dh, nq, nx.maxfd, nx.mani);
        if (!r) r = launch_products(c, h[k], dh, nq, nx.maxfd, nx.mani);
        return r;
      };
      rc = launch_proposals(c, h[0], pd, pa, st.mani);
      hipError_t he = hipSuccess;
      if (!rc) he = hipEventRecord(c->pipe_ev[0], env.stream);
      if (!rc && he == hipSuccess) he = hipStreamWaitEvent(c->stream2, c->pipe_ev[0], 0);
      if (!rc && he == hipSuccess) {
        rc = launch_proposals(c, h[1], pd + pa, st.n - pa, st.mani);
        if (!rc) rc = half(1);
        if (!rc) he = hipEventRecord(c->pipe_ev[1], c->stream2);
      }
      if (!rc && he == hipSuccess) rc = half(0);
      if (!rc && he == hipSuccess) he = hipStreamWaitEvent(env.stream, c->pipe_ev[1], 0);
      if (he != hipSuccess) return fail(NBP_ERR_HIP, std::string("two-stream round: ") + hipGetErrorString(he));
      s++;  // the products ran here
    } else if (st.kind == NBP_STAGE_PROPOSALS) {
      rc = launch_proposals(c, env, (const nbp_proposal_desc *)(p->dev + st.offset), st.n, st.mani);
    } else if (st.kind == NBP_STAGE_PRODUCTS) {
      const nbp_product_desc *dd = (const nbp_product_desc *)(p->dev + st.offset);
      // (fused_second: only a range that starts between the two stages of a fused pair gets here -- three-launch form, the
      //  proposals' fits beside the KD builds, the outputs the fused launch would have fitted behind the products)
      if (st.need_prep || st.fused_second) rc = launch_prep(c, env, fits_dev(st.ent, p->dev), dd, st.n, st.maxfd, st.mani);
      if (!rc) rc = launch_products(c, env, dd, st.n, st.maxfd, st.mani);
      if (!rc && st.fused_second) rc = launch_bandwidth(c, env, fits_dev(st.split_out, p->dev));
    } else if (st.kind == NBP_STAGE_DECONV) {
      rc = launch_deconv(c, (const nbp_proposal_desc *)(p->dev + st.offset), nullptr, st.n);
    } else {
      rc = launch_copies(c, (const nbp_copy_desc *)(p->dev + st.offset), st.n, st.kind == NBP_STAGE_COPY_POINTS);
    }
    if (rc) return rc;
  }
  // leave every slot consistent: run whatever is still pending at the end of the range
  return launch_bandwidth(c, env, fits_dev(p->stages[last].ent, p->dev));
}

nbp_status nbp_program_run(nbp_program *p, int32_t first, int32_t last) {
  if (!p) return fail(NBP_ERR_ARG, "null argument");
  PROG_ALIVE(p);
  if (!p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  nbp_ctx *c = p->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int nuser = p->n_user_stages;
  if (last < 0 || last > nuser) last = nuser;
  if (first < 0) first = 0;
  // (a range that splits a fused variable update -- a PROPOSALS stage and the PRODUCTS stage behind it -- runs that pair in
  //  the three-launch form: run_range)
  // Replay: the launch sequence of a range is captured into a hipGraph the second time it runs and launched as one
  // graph from then on (the descriptors live in device memory, so nbp_program_reseed still takes effect).  Per-kernel
  // event timing (nbp_timing_enable) and programs of a handful of launches take the plain path.
  if (c->timing || !p->use_graph || last - first < 4) return run_range(p, first, last);
  const uint64_t key = ((uint64_t)(uint32_t)first << 32) | (uint32_t)last;
  auto it = p->graphs.find(key);
  if (it != p->graphs.end() && it->second.ws_gen != c->ws_gen) {
    // a workspace was re-allocated since the capture (another program finalized on this context, an immediate-mode
    // call with a larger batch, a clique call): the graph's kernel nodes hold the freed pointer -- capture again
    HIPCHK(hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(it->second.exec);
    p->graphs.erase(it);
    it = p->graphs.end();
  }
  if (it == p->graphs.end() && p->runs[key]++ == 0) return run_range(p, first, last);  // a program that runs once never pays for a capture
  if (it == p->graphs.end()) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    // (relaxed: nothing between begin and end is a call the capture could not take, and under the thread-local mode another
    //  host thread synchronising ITS context's stream meanwhile was refused with "operation not permitted when stream is
    //  capturing" -- seen in round 6 when concurrent callers' clique programs began to be replayed, tools/exp/plan_cache_repro.sh)
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    nbp_status rc = run_range(p, first, last);
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) {  // capture is not available: run directly from now on
      (void)hipGetLastError();
      p->use_graph = false;
      return run_range(p, first, last);
    }
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p->use_graph = false;
      return run_range(p, first, last);
    }
    it = p->graphs.emplace(key, nbp_program::captured{ge, c->ws_gen}).first;
  }
  HIPCHK(hipGraphLaunch(it->second.exec, c->stream));
  return NBP_OK;
  // asynchronous: nbp_synchronize / nbp_slot_read wait for completion
}

nbp_status nbp_program_reseed(nbp_program *p, uint64_t salt) {
  if (!p || !p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  PROG_ALIVE(p);
  nbp_ctx *c = p->ctx;
  HIPCHK(hipSetDevice(c->device));
  (void)hipGetLastError();
  // (the seed fields of a sink's gathered copies stand behind the table's own entries and are re-keyed like their originals)
  if (p->n_seeds > 0)
    hipLaunchKernelGGL(nbp_reseed_kernel, dim3((p->n_seeds + p->n_dup + 255) / 256), dim3(256), 0, c->stream, p->dev,
                       (const int64_t *)(p->dev + p->seed_off), p->n_seeds + p->n_dup, salt);
  HIPCHK(hipGetLastError());
  return NBP_OK;
}

// New seeds for every op of a finalized program (the native host's plan cache: a batch of clique requests whose structure has not
// changed is the same program with other seeds).  `seeds` in stage order: per proposal / deconvolution descriptor its seed and,
// where the descriptor names a stored measurement (meas_seed != 0 when the program was finalized), that one behind it; per
// product descriptor its seed -- the order in which the caller added the stages and their descriptors, which is the order of the
// program's seed table (layout_blob), also where a two-stream round has reordered its descriptors.  Stream-ordered: behind what
// the program has queued so far, in front of its next run.
// Entries [n, n + ndup) of the table are the seed fields of a sink's gathered copies: each takes the value of the entry it follows.
__global__ void nbp_setseed_kernel(char *blob, const int64_t *seed_off, const uint64_t *vals, int n, const int32_t *dup_src, int ndup) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n + ndup) *(uint64_t *)(blob + seed_off[i]) = vals[i < n ? i : dup_src[i - n]];
}
nbp_status nbp_program_num_seeds(nbp_program *p, int32_t *out) {
  if (!p || !out) return fail(NBP_ERR_ARG, "null argument");
  if (!p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  *out = p->n_seeds;
  return NBP_OK;
}
nbp_status nbp_program_set_seeds(nbp_program *p, const uint64_t *seeds, int32_t n) {
  if (!p || !p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  PROG_ALIVE(p);
  if (n != p->n_seeds || (n > 0 && !seeds)) return fail(NBP_ERR_ARG, "set_seeds: the count is not the program's (nbp_program_num_seeds)");
  if (n == 0) return NBP_OK;
  nbp_ctx *c = p->ctx;
  HIPCHK(hipSetDevice(c->device));
  // (from a pinned buffer of the context's pool: a copy from pageable memory would make the caller wait for the stream)
  nbp_ctx::pin_buf *b = pin_acquire(c, (size_t)n * 8);
  if (!b) return fail(NBP_ERR_HIP, "pinned staging buffer");
  memcpy(b->p, seeds, (size_t)n * 8);
  const hipError_t e = hipMemcpyAsync(p->dev + p->seed_val_off, b->p, (size_t)n * 8, hipMemcpyHostToDevice, c->stream);
  pin_release_behind_stream(c, b);
  if (e != hipSuccess) return fail(NBP_ERR_HIP, std::string("hipMemcpyAsync (seeds): ") + hipGetErrorString(e));
  (void)hipGetLastError();
  hipLaunchKernelGGL(nbp_setseed_kernel, dim3((n + p->n_dup + 255) / 256), dim3(256), 0, c->stream, p->dev, (const int64_t *)(p->dev + p->seed_off),
                     (const uint64_t *)(p->dev + p->seed_val_off), n, (const int32_t *)(p->dev + p->dup_src_off), p->n_dup);
  HIPCHK(hipGetLastError());
  return NBP_OK;
}

// order[i] = where, in a walk over the program's descriptors as they lie in its blob, the seed field seeds[i] goes to: 0, 1, 2 ...
// unless a two-stream round moved descriptors (what tests ask to know that a round they made really is reordered)
nbp_status nbp_program_seed_order(nbp_program *p, int32_t *order, int32_t n) {
  if (!p || !p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  if (n != p->n_seeds || (n > 0 && !order)) return fail(NBP_ERR_ARG, "seed_order: the count is not the program's (nbp_program_num_seeds)");
  if (n > 0) memcpy(order, p->seed_rank.data(), (size_t)n * sizeof(int32_t));
  return NBP_OK;
}

nbp_status nbp_program_num_stages(nbp_program *p, int32_t *out) {
  if (!p || !out) return fail(NBP_ERR_ARG, "null argument");
  *out = p->finalized ? p->n_user_stages : (int32_t)p->stages.size();
  return NBP_OK;
}

nbp_status nbp_program_num_fused(nbp_program *p, int32_t *out) {
  if (!p || !out) return fail(NBP_ERR_ARG, "null argument");
  int n = 0;
  for (const nbp_stage &st : p->stages) n += st.fused ? 1 : 0;
  *out = n;
  return NBP_OK;
}

nbp_status nbp_program_num_two_stream(nbp_program *p, int32_t *out) {
  if (!p || !out) return fail(NBP_ERR_ARG, "null argument");
  int n = 0;
  for (const nbp_stage &st : p->stages) n += st.pipe ? 1 : 0;
  *out = n;
  return NBP_OK;
}

nbp_status nbp_program_lane_plan(nbp_program *p, nbp_lane_part_rec *out, int32_t cap, int32_t *n_out) {
  if (!p || !n_out || (!out && cap > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (!p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  const int np = p->parts.empty() ? 0 : (int)p->parts.size() - 1;  // (without the trailing pseudo part)
  *n_out = np;
  for (int k = 0; k < np && k < cap; k++) {
    const nbp_stage &st = p->parts[(size_t)k];
    const nbp_stage &us = p->stages[(size_t)st.user];
    const size_t esz = st.kind == NBP_STAGE_PRODUCTS ? sizeof(nbp_product_desc) : (st.kind == NBP_STAGE_COPIES || st.kind == NBP_STAGE_COPY_POINTS ?
                       sizeof(nbp_copy_desc) : sizeof(nbp_proposal_desc));
    out[k] = {st.user, st.lane, st.gathered ? 0 : (int32_t)((st.offset - us.offset) / esz), st.n, st.waits.empty() ? -1 : st.waits[0], st.signals ? 1 : 0};
  }
  return NBP_OK;
}

nbp_status nbp_program_sink_plan(nbp_program *p, int32_t *gained, int32_t cap, int32_t *n_out) {
  if (!p || !n_out || (!gained && cap > 0)) return fail(NBP_ERR_ARG, "null argument");
  if (!p->finalized) return fail(NBP_ERR_ARG, "program not finalized");
  const int np = p->parts.empty() ? 0 : (int)p->parts.size() - 1;
  *n_out = np;
  for (int k = 0; k < np && k < cap; k++) gained[k] = p->parts[(size_t)k].gained;
  return NBP_OK;
}

// the programs handed to nbp_program_retire whose last launch has run
static void program_free(nbp_program *p, bool sync);
static void reap_retired(nbp_ctx *c) {
  for (size_t i = 0; i < c->retired.size();) {
    if (hipEventQuery(c->retired[i].second) == hipSuccess) {
      hipEventDestroy(c->retired[i].second);
      nbp_program *p = c->retired[i].first;
      c->retired.erase(c->retired.begin() + (long)i);
      program_free(p, false);
    } else
      i++;
  }
}
// Destroy a program without waiting for it: it is dropped once everything queued on the library stream up to now has run
// (checked at the next retire / nbp_clique_submit_batch / nbp_synchronize; nbp_ctx_destroy takes what is left).  Its device
// blob goes to the next short-lived program only then.
nbp_status nbp_program_retire(nbp_program *p) {
  if (!p) return NBP_OK;
  if (!p->ctx) { delete p; return NBP_OK; }
  nbp_ctx *c = p->ctx;
  hipSetDevice(c->device);
  reap_retired(c);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, c->stream) != hipSuccess) {
    if (ev) hipEventDestroy(ev);
    return nbp_program_destroy(p);  // (waits instead)
  }
  c->retired.emplace_back(p, ev);
  return NBP_OK;
}
nbp_status nbp_program_destroy(nbp_program *p) {
  if (!p) return NBP_OK;
  program_free(p, true);
  return NBP_OK;
}
static void program_free(nbp_program *p, bool sync) {
  if (p->ctx) {  // (a program whose context is gone was detached by nbp_ctx_destroy: nothing left on the device)
    hipSetDevice(p->ctx->device);
    if (sync) hipStreamSynchronize(p->ctx->stream);
    if (p->dev) {
      // small blobs are kept for the next program of this context (hipFree synchronises the whole device)
      auto &bc = p->ctx->blob_cache;
      // (a queued walk retires one program per tree level and direction before the first of them has run: room for all of them)
      if (p->dev_bytes <= (16u << 20) && bc.size() < 64) bc.emplace_back(p->dev, p->dev_bytes);
      else hipFree(p->dev);
    }
    for (auto &kv : p->graphs) hipGraphExecDestroy(kv.second.exec);
    auto &v = p->ctx->programs;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i] == p) { v.erase(v.begin() + i); break; }
  }
  delete p;
}

// ---- separator exchange between ranks: RCCL point-to-point over xGMI, from C -----------------------------------------
// The messages of a tree solve are single slots (4.9 KB at N = 200) on the few tree edges that cross a rank boundary:
// latency-bound traffic, so all messages of one exchange point go into ONE ncclGroupStart / ncclGroupEnd of ncclSend /
// ncclRecv on the library's own stream -- stream-ordered with the kernels that produce and consume the slots, no host
// synchronisation, no ring collective.  RCCL is bound at run time (dlopen + dlsym): a process that already has RCCL loaded
// (PyTorch brings its own) keeps exactly one copy, and libnbp.so has no link-time dependency on it.
struct rccl_api {
  void *h = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclCommUserRank) CommUserRank = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static rccl_api g_rccl;
static nbp_status rccl_load() {
  if (g_rccl.Send) return NBP_OK;
  const char *env = getenv("NBP_RCCL_LIB");
  const char *names[] = {env, "librccl.so", "librccl.so.1"};
  void *h = nullptr;
  for (const char *n : names)  // a copy that is already mapped first
    if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
  for (const char *n : names)
    if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(NBP_ERR_HIP, std::string("RCCL not found (librccl.so): ") + (dlerror() ? dlerror() : ""));
  g_rccl.h = h;
#define NBP_RCCL_SYM(F) g_rccl.F = (decltype(g_rccl.F))dlsym(h, "nccl" #F); if (!g_rccl.F) return fail(NBP_ERR_HIP, "RCCL: missing symbol nccl" #F)
  NBP_RCCL_SYM(GetUniqueId);
  NBP_RCCL_SYM(CommInitRank);
  NBP_RCCL_SYM(CommDestroy);
  NBP_RCCL_SYM(CommCount);
  NBP_RCCL_SYM(CommUserRank);
  NBP_RCCL_SYM(GroupStart);
  NBP_RCCL_SYM(GroupEnd);
  NBP_RCCL_SYM(Recv);
  NBP_RCCL_SYM(GetErrorString);
  NBP_RCCL_SYM(Send);
#undef NBP_RCCL_SYM
  return NBP_OK;
}
#define RCCLCHK(expr)                                                                                  \
  do {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                          \
    if (r_ != ncclSuccess) return fail(NBP_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)

struct nbp_comm {
  ncclComm_t comm = nullptr;
  nbp_ctx *ctx = nullptr;  // null once the context is gone (nbp_ctx_destroy shuts the communicator down first)
  int world = 0, rank = 0;
};
static void comm_shutdown(nbp_comm *m) {
  if (m->comm && m->ctx && g_rccl.CommDestroy) {
    hipSetDevice(m->ctx->device);
    hipStreamSynchronize(m->ctx->stream);
    g_rccl.CommDestroy(m->comm);
  }
  m->comm = nullptr;
  m->ctx = nullptr;
}
// called by nbp_ctx_destroy while the stream still exists
static void ctx_detach_comms(nbp_ctx *c) {
  for (nbp_comm *m : c->comms) comm_shutdown(m);
  c->comms.clear();
}

nbp_status nbp_comm_unique_id(void *id_out) {
  if (!id_out) return fail(NBP_ERR_ARG, "null argument");
  nbp_status rc = rccl_load();
  if (rc) return rc;
  ncclUniqueId id;
  RCCLCHK(g_rccl.GetUniqueId(&id));
  memcpy(id_out, &id, NBP_COMM_ID_BYTES);
  return NBP_OK;
}

nbp_status nbp_comm_create(nbp_ctx *c, int32_t world, int32_t rank, const void *id, nbp_comm **out) {
  if (!c || !id || !out) return fail(NBP_ERR_ARG, "null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(NBP_ERR_RANGE, "comm: rank / world");
  nbp_status rc = rccl_load();
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId uid;
  static_assert(sizeof(uid) == NBP_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(&uid, id, sizeof(uid));
  nbp_comm *m = new nbp_comm();
  m->ctx = c; m->world = world; m->rank = rank;
  ncclResult_t r = g_rccl.CommInitRank(&m->comm, world, uid, rank);
  if (r != ncclSuccess) { delete m; return fail(NBP_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
  c->comms.push_back(m);
  *out = m;
  return NBP_OK;
}

nbp_status nbp_comm_destroy(nbp_comm *m) {
  if (!m) return NBP_OK;
  if (m->ctx) {
    auto &v = m->ctx->comms;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i] == m) { v.erase(v.begin() + i); break; }
  }
  comm_shutdown(m);  // nothing left to do when the context went first
  delete m;
  return NBP_OK;
}

nbp_status nbp_comm_info(nbp_comm *m, int32_t *nranks_out, int32_t *rank_out) {
  if (!m || !nranks_out || !rank_out) return fail(NBP_ERR_ARG, "null argument");
  if (!m->ctx || !m->comm) return fail(NBP_ERR_ARG, "comm_info: the communicator's context was destroyed");
  int n = 0, r = 0;
  RCCLCHK(g_rccl.CommCount(m->comm, &n));
  RCCLCHK(g_rccl.CommUserRank(m->comm, &r));
  *nranks_out = n;
  *rank_out = r;
  return NBP_OK;
}

// ---- self-test of the shared elementary functions (include/nbp_math.h) on the device -----------------------------------
__global__ void nbp_math_eval_kernel(int fn, const double *a, const double *b, double *o0, double *o1, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r0 = 0.0, r1 = 0.0;
  switch (fn) {
  case 0: r0 = nbpm_log(a[i]); break;
  case 1: nbpm_sincos(a[i], &r0, &r1); break;
  case 2: r0 = nbpm_atan2(a[i], b[i]); break;
  case 3: r0 = nbpm_wrap_pi(a[i]); break;
  default: nbpm_box_muller(a[i], b[i], &r0, &r1); break;
  }
  o0[i] = r0;
  if (o1) o1[i] = r1;
}
nbp_status nbp_math_eval(nbp_ctx *c, int32_t fn, const double *a, const double *b, double *out0, double *out1, int64_t n) {
  if (!c || !a || !out0) return fail(NBP_ERR_ARG, "null argument");
  if (fn < 0 || fn > 4) return fail(NBP_ERR_RANGE, "math_eval: fn");
  if ((fn == 2 || fn == 4) && !b) return fail(NBP_ERR_ARG, "math_eval: this function takes two arguments");
  if (n <= 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  double *d = nullptr;
  HIPCHK(hipMalloc(&d, sizeof(double) * 4 * (size_t)n));
  nbp_status rc = NBP_OK;
  do {
    if (hipMemcpyAsync(d, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(NBP_ERR_HIP, "math_eval: copy in"); break; }
    if (b && hipMemcpyAsync(d + n, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(NBP_ERR_HIP, "math_eval: copy in"); break; }
    hipLaunchKernelGGL(nbp_math_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (int)fn, d, b ? d + n : nullptr, d + 2 * n, d + 3 * n, (long long)n);
    if (hipMemcpyAsync(out0, d + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { rc = fail(NBP_ERR_HIP, "math_eval: copy out"); break; }
    if (out1 && hipMemcpyAsync(out1, d + 3 * n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { rc = fail(NBP_ERR_HIP, "math_eval: copy out"); break; }
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(NBP_ERR_HIP, "math_eval: synchronize");
  } while (0);
  hipFree(d);
  return rc;
}

nbp_status nbp_exchange(nbp_ctx *c, nbp_comm *m, const nbp_xfer *sends, int32_t ns, const nbp_xfer *recvs, int32_t nr) {
  if (!c || !m || (ns > 0 && !sends) || (nr > 0 && !recvs)) return fail(NBP_ERR_ARG, "null argument");
  if (!m->ctx || !m->comm) return fail(NBP_ERR_ARG, "exchange: the communicator's context was destroyed");
  if (m->ctx != c) return fail(NBP_ERR_ARG, "exchange: the communicator belongs to another context");
  for (int i = 0; i < ns; i++)
    if (sends[i].peer < 0 || sends[i].peer >= m->world || sends[i].slot < 0 || sends[i].slot >= c->n_slots) return fail(NBP_ERR_RANGE, "exchange: send");
  for (int i = 0; i < nr; i++)
    if (recvs[i].peer < 0 || recvs[i].peer >= m->world || recvs[i].slot < 0 || recvs[i].slot >= c->n_slots) return fail(NBP_ERR_RANGE, "exchange: recv");
  if (ns + nr == 0) return NBP_OK;
  HIPCHK(hipSetDevice(c->device));
  RCCLCHK(g_rccl.GroupStart());
  // a failing Send / Recv must not leave the group open for the rest of the process: close it, then report the first error
  ncclResult_t bad = ncclSuccess;
  const char *what = "";
  for (int i = 0; i < ns && bad == ncclSuccess; i++) {
    bad = g_rccl.Send(c->arena + c->S * sends[i].slot, (size_t)c->S, ncclDouble, sends[i].peer, m->comm, c->stream);
    what = "ncclSend";
  }
  for (int i = 0; i < nr && bad == ncclSuccess; i++) {
    bad = g_rccl.Recv(c->arena + c->S * recvs[i].slot, (size_t)c->S, ncclDouble, recvs[i].peer, m->comm, c->stream);
    what = "ncclRecv";
  }
  const ncclResult_t ge = g_rccl.GroupEnd();
  if (bad != ncclSuccess) return fail(NBP_ERR_HIP, std::string(what) + ": " + g_rccl.GetErrorString(bad));
  if (ge != ncclSuccess) return fail(NBP_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(ge));
  return NBP_OK;  // stream-ordered: the next launch on the library stream sees the received slots
}

// ---- timing / diagnostics -------------------------------------------------------------------------------
nbp_status nbp_timing_enable(nbp_ctx *c, int32_t on) {
  if (!c) return fail(NBP_ERR_ARG, "null argument");
  c->timing = on != 0;
  return NBP_OK;
}
static nbp_status drain(std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, double &ms, int64_t &cnt) {
  for (auto &p : v) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, p.first, p.second));
    ms += t;
    cnt++;
    hipEventDestroy(p.first);
    hipEventDestroy(p.second);
  }
  v.clear();
  return NBP_OK;
}
nbp_status nbp_timing_read(nbp_ctx *c, double *ms, int64_t *launches) {
  return nbp_timing_read_n(c, ms, launches, 4);
}
nbp_status nbp_timing_read_n(nbp_ctx *c, double *ms, int64_t *launches, int32_t n) {
  if (!c) return fail(NBP_ERR_ARG, "null argument");
  if (n < 0 || n > 5) return fail(NBP_ERR_RANGE, "timing: n in [0, 5]");
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 5; k++) {
    nbp_status rc = drain(c->ev[k], c->ms[k], c->nl[k]);
    if (rc) return rc;
    if (k < n && ms) ms[k] = c->ms[k];
    if (k < n && launches) launches[k] = c->nl[k];
    c->ms[k] = 0;
    c->nl[k] = 0;
  }
  return NBP_OK;
}
// ---- launch plans (nbp.h): the planners themselves, on a context that holds only what they read -----------------------
// (ctx_plan_fields + the level table of N; no device, no stream: nothing here touches the GPU)
static nbp_status plan_ctx(nbp_ctx &c, int N) {
  if (N < 8 || N > NBP_MAXN) return fail(NBP_ERR_RANGE, "N must be in [8, 512]");
  std::vector<int32_t> ints;
  std::vector<double> dbls;
  ctx_plan_fields(&c, N);
  return levels_host(N, c.T, ints, dbls);
}
nbp_status nbp_plan_products(const nbp_product_plan_req *req, nbp_product_plan_rec *out, int64_t n) {
  if ((!req || !out) && n > 0) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx c;
  for (int64_t i = 0; i < n; i++) {
    const nbp_product_plan_req &q = req[i];
    if (c.N != q.N) {  // (requests sorted by N build the level table once per N)
      c = nbp_ctx();
      NBPCHK(plan_ctx(c, q.N));
    }
    if (q.n < 1 || q.F < 1 || q.F > NBP_MAXF || q.D < 1 || q.D > 3 || q.mani < -1 || q.mani > NBP_SE2 || q.geom_n < 0)
      return fail(NBP_ERR_ARG, "plan query: request " + std::to_string(i) + ": out of range");
    nbp_launch_env env;
    env.geom_n = q.geom_n;
    if (q.mani > 0 && manifold_dim_h(q.mani) != q.D) {  // products_maxfd: D is the batch's largest dimension -- its manifold's
      out[i] = nbp_product_plan_rec{};
      out[i].status = NBP_ERR_ARG;
      out[i].row = -1;
      out[i].N = q.N; out[i].n = q.n; out[i].F = q.F; out[i].D = q.D; out[i].mani = q.mani; out[i].geom_n = q.geom_n;
      continue;
    }
    out[i] = product_plan_rec(&c, env, q.n, q.F * 4 + q.D, q.mani, product_plan(&c, env, q.n, q.F * 4 + q.D, q.mani));
  }
  return NBP_OK;
}
nbp_status nbp_plan_fits(const nbp_fit_plan_req *req, nbp_fit_plan_rec *out, int64_t n) {
  if ((!req || !out) && n > 0) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx c;
  for (int64_t i = 0; i < n; i++) {
    const nbp_fit_plan_req &q = req[i];
    if (c.N != q.N) {
      c = nbp_ctx();
      NBPCHK(plan_ctx(c, q.N));
    }
    if (q.fits < 0 || q.coords < 0 || q.products < 0 || q.kdF < 0 || q.geom_blocks < 0 || (q.fits == 0 && q.products == 0))
      return fail(NBP_ERR_ARG, "plan query: request " + std::to_string(i) + ": out of range");
    nbp_launch_env env;
    env.geom_blocks = q.geom_blocks;
    env.geom_n = q.geom_blocks ? std::max(q.products, 1) : 0;  // (a round sets both; the fit plan reads geom_n as a flag)
    const bool prep = q.products > 0;
    out[i] = fit_plan_rec(&c, env, q.fits, q.coords, q.products, q.kdF, prep, fit_plan(&c, env, q.fits, q.coords, q.products, q.kdF));
  }
  return NBP_OK;
}
nbp_status nbp_plan_proposals(const nbp_proposal_plan_req *req, nbp_proposal_plan_rec *out, int64_t n) {
  if ((!req || !out) && n > 0) return fail(NBP_ERR_ARG, "null argument");
  nbp_ctx c;
  for (int64_t i = 0; i < n; i++) {
    const nbp_proposal_plan_req &q = req[i];
    if (c.N != q.N) {
      c = nbp_ctx();
      NBPCHK(plan_ctx(c, q.N));
    }
    if (q.n < 1 || q.manifold < 0 || q.manifold > NBP_SE2) return fail(NBP_ERR_ARG, "plan query: request " + std::to_string(i) + ": out of range");
    const int M = q.manifold;  // (the classes of proposals_uniform_class; Euclid(1) has none)
    const int cls = M == NBP_EUCLID2 ? NBP_CLS_LIN2 : (M == NBP_EUCLID3 ? NBP_CLS_LIN3 : (M == NBP_CIRCULAR ? NBP_CLS_CIRC : (M == NBP_SE2 ? NBP_CLS_SE2 : 0)));
    const nbp_proposal_plan p = proposal_plan(&c, q.n, cls | ((cls && q.simple) ? NBP_CLS_SIMPLE : 0));
    nbp_proposal_plan_rec r{};
    r.status = NBP_OK;
    r.geometry = p.geometry; r.blocks = p.blocks; r.threads = p.threads;
    r.N = q.N; r.n = q.n; r.manifold = q.manifold; r.simple = q.simple;
    r.lds = (int64_t)p.lds;
    snprintf(r.kernel, sizeof(r.kernel), "%s", p.name);
    out[i] = r;
  }
  return NBP_OK;
}
nbp_status nbp_last_plans(nbp_ctx *c, nbp_product_plan_rec *product, nbp_fit_plan_rec *prep, nbp_fit_plan_rec *fits) {
  if (!c) return fail(NBP_ERR_ARG, "ctx is null");
  if (product) *product = c->last_product;
  if (prep) *prep = c->last_prep;
  if (fits) *fits = c->last_fit;
  return NBP_OK;
}

nbp_status nbp_diag_read(nbp_ctx *c, nbp_diag *out, int32_t reset) {
  if (!c || !out) return fail(NBP_ERR_ARG, "null argument");
  nbp_counters h;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(&h, c->counters, sizeof(h), hipMemcpyDeviceToHost));
  out->solves = (int64_t)h.solves;
  out->nonconverged = (int64_t)h.nonconverged;
  out->nan_results = (int64_t)h.nan_results;
  out->residual_evals = (int64_t)h.residual_evals;
  out->lcv_evals = (int64_t)h.lcv_evals;
  out->lcv_evals_f32 = (int64_t)h.lcv_evals_f32;
  out->proposal_launches_workgroup = c->prop_launches[0];
  out->proposal_launches_wave = c->prop_launches[1];
  out->proposal_launches_split = c->prop_launches[2];
  if (reset) c->prop_launches[0] = c->prop_launches[1] = c->prop_launches[2] = 0;
  out->lane_side_launches = c->lane_side_launches;
  out->lane_waits = c->lane_waits;
  out->lane_side_updates = c->lane_side_updates;
  if (reset) c->lane_side_launches = c->lane_waits = c->lane_side_updates = 0;
  out->sunk_updates = c->sunk_updates;
  out->sink_launches = c->sink_launches;
  if (reset) c->sunk_updates = c->sink_launches = 0;
  if (reset) HIPCHK(hipMemset(c->counters, 0, offsetof(nbp_counters, flags)));  // (the flags are the context's, not counters)
  return NBP_OK;
}

#ifdef NBP_PHASE_TIMING
nbp_status nbp_debug_phase_read(long long *out, int n, int reset) {
  long long h[64];
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(nbp_phase_clk), sizeof(h)));
  for (int i = 0; i < n && i < 64; i++) out[i] = h[i];
  if (reset) {
    memset(h, 0, sizeof(h));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(nbp_phase_clk), h, sizeof(h)));
  }
  return NBP_OK;
}
nbp_status nbp_debug_block_read(long long *out, int nblocks) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(nbp_block_clk), sizeof(long long) * 3 * (size_t)(nblocks < 8192 ? nblocks : 8192)));
  return NBP_OK;
}
nbp_status nbp_debug_block_hist(unsigned int *out, int reset) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(nbp_block_hist), sizeof(unsigned int) * 4 * 64));
  if (reset) {
    unsigned int z[4 * 64] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(nbp_block_hist), z, sizeof(z)));
  }
  return NBP_OK;
}
#endif

}  // extern "C"
