// Stand-alone check of the launch plans of libnbp over their whole argument space (tests/test_launch_plans.py compiles and runs it).
//   hipcc --offload-arch=gfx950 -std=c++17 -O2 -I include -I incrementalinference.jl_amd/csrc launch_plan_check.cpp -o check -ldl
//   ./check incrementalinference.jl_amd/csrc/libnbp.so
// The plans come from the library's own planners through nbp_plan_products / nbp_plan_fits / nbp_plan_proposals (include/nbp.h: no
// context, no GPU); what a kernel addresses of its LDS is computed HERE, from the kernels' own header, the way the kernels call
// product_lds_layout (product_body, product_kernel_uniform in nbp_kernels.h).  The plan and the kernel meet only at run time: an
// LDS overrun does not fault, it gives wrong or non-finite posteriors.
//
// Swept for products: every N in 8..512; n in {1, 15, 16, 191, 192, 256, 257, 512, 513, 5000}; F in 1..128; D in 1..3; mani in
// {-1, 0, 1..5}; geom_n in {0, n}; under the option sets OPTION_SETS below (the library reads them when a plan is queried, as it
// does when a context is created).  Exit status 0: every invariant holds; the counts are printed either way.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#define NBP_TU 0  // declarations of the kernels only
#include "nbp_kernels.h"

typedef nbp_status (*plan_products_fn)(const nbp_product_plan_req *, nbp_product_plan_rec *, int64_t);
typedef nbp_status (*plan_fits_fn)(const nbp_fit_plan_req *, nbp_fit_plan_rec *, int64_t);
typedef nbp_status (*plan_proposals_fn)(const nbp_proposal_plan_req *, nbp_proposal_plan_rec *, int64_t);
static plan_products_fn plan_products;
static plan_fits_fn plan_fits;
static plan_proposals_fn plan_proposals;
static const char *(*last_error)(void);

static const size_t LDS_BYTES = 160 * 1024;     // LDS of a CU of gfx950: what a workgroup can be given at most
static const int PROPOSAL_LDS_CAP = 64 * 1024;  // dynamic LDS of a kernel that has not asked for more (the proposal kernels)
static const int CUS = 256;                     // CUs of the chip: the `_w1` kernels are compiled for one workgroup per CU
// the speculative fits: rendezvous areas of a context / workgroups that are resident at once (NBP_SPEC_MAXJOBS, NBP_SPEC_MAXBLOCKS)
static const int SPEC_MAXJOBS = 40, SPEC_MAXBLOCKS = 224;

static int mani_dim(int m) { return m == NBP_SE2 ? 3 : (m == NBP_CIRCULAR ? 1 : m); }

// the tree of N leaves: nodes of all levels (TOT = T.off[T.L] + T.cnt[T.L] in the kernels) -- every level halves each node of
// more than one leaf, a leaf stays
static int tree_total(int N) {
  std::vector<int> cur{N};
  int total = 0;
  for (;;) {
    total += (int)cur.size();
    bool all_leaf = true;
    std::vector<int> nxt;
    for (int w : cur) {
      if (w > 1) { all_leaf = false; nxt.push_back((w + 1) / 2); nxt.push_back(w - (w + 1) / 2); }
      else nxt.push_back(w);
    }
    if (all_leaf) break;
    cur.swap(nxt);
  }
  return total;
}

// bytes of dynamic LDS the kernel of plan `r` addresses for a product of Fp densities on a manifold of dimension Dp
static size_t kernel_lds_need(const nbp_product_plan_rec &r, int Fp, int Dp, int TOT) {
  const int N = r.N, HL = r.row_HL, TB = r.wpb * 64, SPB = TB / HL;
  const size_t CK = HL <= 4 ? (size_t)r.nch * 2 * TB : 0;  // CKL of product_body (FUSED != 1 in every product kernel)
  if (r.row_mani == 0) {
    // product_kernel_body: BIG (HL >= 8 and a scratch area) = product_body's defaults: one level at a time, no chunk area, circ rows
    if (r.big) return product_lds_layout(Fp, Dp, N, SPB, true, nullptr, nullptr, N, 0, true);
    return product_lds_layout(Fp, Dp, N, SPB, false, nullptr, nullptr, r.all_levels ? TOT : N, CK, true);
  }
  // product_kernel_uniform<MANI, HL, XS>
  const bool lay_circ = HL >= 8 || r.row_mani == NBP_CIRCULAR || r.row_mani == NBP_SE2;
  const size_t own = product_lds_layout(Fp, Dp, N, SPB, false, nullptr, nullptr, r.all_levels ? TOT : N, CK, lay_circ);
  if (!r.row_xs) return own;
  return (own + 7) / 8 * 8 + nbp_product_xs_doubles(Fp, Dp, N) * 8;  // xs, cen, bw behind the product's own areas
}

struct tally {
  long plans = 0, ok = 0, refused[4] = {0, 0, 0, 0}, invalid = 0, sizing = 0, oversize = 0, failures = 0;
  std::set<std::tuple<int, int, int, int, int, int, int>> sigs;  // (row, big, nch, all_levels, wpb, G > 1, circ) of the launched plans
  std::set<int> rows;
  std::vector<std::string> msgs, over_msgs;
  void fail(const char *what, const nbp_product_plan_rec &r) {
    failures++;
    if (msgs.size() < 21) {
      char b[512];
      snprintf(b, sizeof(b), "%s: N=%d n=%d F=%d D=%d mani=%d geom_n=%d -> HL=%d wpb=%d G=%d big=%d xs=%d nch=%d all=%d w1=%d row=%d(%s) lds=%ld gstats=%ld status=%d/%d",
               what, r.N, r.n, r.F, r.D, r.mani, r.geom_n, r.HL, r.wpb, r.G, r.big, r.xs, r.nch, r.all_levels, r.w1, r.row, r.kernel, (long)r.lds,
               (long)r.gstats, r.status, r.refusal);
      msgs.push_back(b);
    }
  }
  void merge(const tally &o) {
    plans += o.plans; ok += o.ok; invalid += o.invalid; sizing += o.sizing; oversize += o.oversize; failures += o.failures;
    for (int i = 0; i < 4; i++) refused[i] += o.refused[i];
    sigs.insert(o.sigs.begin(), o.sigs.end());
    rows.insert(o.rows.begin(), o.rows.end());
    for (const std::string &m : o.msgs) if (msgs.size() < 20) msgs.push_back(m);
    for (const std::string &m : o.over_msgs) if (over_msgs.size() < 5) over_msgs.push_back(m);
  }
};

static const int NS[] = {1, 15, 16, 191, 192, 256, 257, 512, 513, 5000};
static const int MANIS[] = {-1, 0, 1, 2, 3, 4, 5};

static void check_products_of(int N, tally &t) {
  const int TOT = tree_total(N);
  std::vector<nbp_product_plan_req> req;
  for (int n : NS)
    for (int F = 1; F <= 128; F++)
      for (int D = 1; D <= 3; D++)
        for (int mani : MANIS)
          for (int g = 0; g < 2; g++) req.push_back({N, n, F, D, mani, g ? n : 0});
  std::vector<nbp_product_plan_rec> rec(req.size());
  if (plan_products(req.data(), rec.data(), (int64_t)req.size()) != NBP_OK) {
    fprintf(stderr, "nbp_plan_products failed at N = %d: %s\n", N, last_error());
    exit(2);
  }
  // the halves of a two-stream round (geom_n = n): launches of fewer products under the geometry of the whole batch
  std::vector<nbp_product_plan_req> hreq;
  std::vector<size_t> hof;
  for (size_t i = 0; i < req.size(); i++)
    if (req[i].geom_n && rec[i].status != NBP_ERR_ARG)
      for (int h : {1, req[i].n / 2, req[i].n - 1})
        if (h >= 1 && h < req[i].n) { nbp_product_plan_req q = req[i]; q.n = h; hreq.push_back(q); hof.push_back(i); }
  std::vector<nbp_product_plan_rec> hrec(hreq.size());
  if (!hreq.empty() && plan_products(hreq.data(), hrec.data(), (int64_t)hreq.size()) != NBP_OK) exit(2);
  for (size_t k = 0; k < hreq.size(); k++) {
    const nbp_product_plan_rec &w = rec[hof[k]], &h = hrec[k];
    if (h.HL != w.HL || h.wpb != w.wpb || h.G != w.G || h.nch != w.nch || h.lds != w.lds || h.xs != w.xs || h.big != w.big || h.all_levels != w.all_levels || h.row != w.row)
      t.fail("a half of a round does not take the geometry of the whole batch", h);
  }
  for (size_t i = 0; i < rec.size(); i++) {
    const nbp_product_plan_rec &r = rec[i];
    t.plans++;
    if (r.status == NBP_ERR_ARG) {  // D is not the dimension of the launch's single manifold: no launch has such arguments (products_maxfd)
      if (!(r.mani > 0 && mani_dim(r.mani) != r.D)) t.fail("query refused arguments a launch can have", r);
      t.invalid++;
      continue;
    }
    if (r.N != req[i].N || r.n != req[i].n || r.F != req[i].F || r.D != req[i].D || r.mani != req[i].mani || r.geom_n != req[i].geom_n) t.fail("the record does not echo the request", r);
    const int TB = r.wpb * 64, SPB = r.HL > 0 ? TB / r.HL : 0;
    // ---- geometry (of every plan, launched or refused) ----
    if (!(r.HL == 32 || r.HL == 8 || r.HL == 2)) { t.fail("helper lanes", r); continue; }
    if (!((long)r.G * SPB >= r.N && r.N > (long)(r.G - 1) * SPB)) t.fail("G * SPB >= N > (G - 1) * SPB", r);
    if (r.HL <= 4 && (r.wpb & 3)) t.fail("throughput workgroup is not a multiple of four waves", r);
    // (inside a round the plan keeps the geometry of the whole batch whatever it is, and big is refused there: the next line)
    const bool big_refused = r.refusal == NBP_PLAN_REFUSED_BIG_IN_ROUND;
    if (r.big && r.HL != 8 && !big_refused) t.fail("big outside HL = 8", r);
    if (r.big ? r.gstats != (int64_t)((size_t)r.n * r.G * nbp_product_gstats_doubles(r.F, 3, r.N)) : r.gstats != 0) t.fail("gstats", r);
    if (r.big && r.geom_n && r.refusal != NBP_PLAN_REFUSED_BIG_IN_ROUND) t.fail("big inside a round is not refused", r);
    if (r.w1 && !((long)r.n * r.G <= CUS && TB <= 256 && !r.geom_n)) t.fail("_w1 beyond one workgroup of four waves per CU, or inside a round", r);
    if (r.nch && !(r.HL <= 4 && !r.big)) t.fail("chunk sums outside the throughput geometry", r);
    if (r.HL <= 4 && !r.big && !(r.nch >= 1 && r.nch <= 15)) t.fail("chunks per helper range (four bits of the kernel argument)", r);
    if (r.xs && !(r.HL <= 4 && r.mani > 0 && !r.big && r.F <= NBP_FUSED_MAXF)) t.fail("_xs outside the single-manifold throughput kernels", r);
    // ---- status ----
    if (r.status == NBP_OK) {
      if (r.refusal || r.row < 0) t.fail("NBP_OK without a kernel", r);
    } else if (r.status == NBP_ERR_RANGE) {
      if (r.refusal < 1 || r.refusal > 3) t.fail("an undefined refusal", r);
      // (launch_products tests the LDS before the table: NO_KERNEL is by construction a plan whose LDS fits, and none may exist)
      if (r.refusal == NBP_PLAN_REFUSED_NO_KERNEL) t.fail("no kernel for a geometry whose LDS fits", r);
      if (r.refusal == NBP_PLAN_REFUSED_LDS && (size_t)r.lds <= LDS_BYTES) t.fail("refused for the LDS, which fits", r);
      t.refused[r.refusal & 3]++;
    } else
      t.fail("status", r);
    // mani = -1 is no launch: presize_products asks what the widest workgroup ANY kernel takes would need of the scratch area
    // (its `gstats`), and pairs that geometry with the generic row only for want of another -- geometry and gstats are checked
    // above, the row and the LDS are nobody's
    if (r.mani < 0) { t.sizing++; continue; }
    if (r.row >= 0) {
      if (r.row_HL != r.HL || r.row_xs != r.xs || r.row_w1 != r.w1) t.fail("the row is not the plan's", r);
      if (r.row_mani != 0 && r.row_mani != r.mani) t.fail("a single-manifold row for another batch", r);
      if (r.big && r.row_mani != 0 && !big_refused) t.fail("big on a single-manifold row (they have no scratch path)", r);
      if (TB > r.launch_bound) t.fail("workgroup beyond the kernel's launch bound", r);
    }
    if (r.status != NBP_OK) continue;
    // ---- the launched plans: the LDS ----
    t.ok++;
    t.rows.insert(r.row);
    t.sigs.insert(std::make_tuple(r.row, r.big, r.nch, r.all_levels, r.wpb, r.G > 1, r.circ));
    if ((size_t)r.lds > LDS_BYTES) t.fail("launched with more than 160 KB of LDS", r);
    // every product of the launch: 2 .. F densities (F = 1 is no launch's largest: swept, and then the plan's own F), on the
    // launch's manifold, or in a mixed launch on any manifold of up to D dimensions
    size_t need = 0;
    for (int Fp = r.F < 2 ? r.F : 2; Fp <= r.F; Fp++)
      for (int Dp = r.row_mani ? r.D : 1; Dp <= r.D; Dp++) {
        const size_t nd = kernel_lds_need(r, Fp, Dp, TOT);
        if (nd > need) need = nd;
      }
    if ((size_t)r.lds < need) t.fail("the kernel addresses more LDS than the launch allocates", r);
    else {
      // exactly the need at the largest F -- an oversize plan quietly costs residency.  (The _xs kernels start their coordinates at
      // the next multiple of eight bytes behind the product's own areas, which end on a multiple of four; the plan allows eight
      // bytes for it instead of rounding: up to eight bytes of slack there are the alignment, not an oversize.)
      const size_t slack = (size_t)r.lds - kernel_lds_need(r, r.F, r.D, TOT);
      if (slack > (r.row_xs ? 8u : 0u)) {
        t.oversize++;
        if (t.over_msgs.size() < 5) { t.fail("(oversize) more LDS than the kernel addresses at the largest F", r); t.failures--; t.over_msgs.push_back(t.msgs.back()); t.msgs.pop_back(); }
      }
    }
  }
}

static void check_fits_of(int N, long &plans, long &failures, std::set<std::tuple<std::string, int, int, int>> &sigs, std::vector<std::string> &msgs) {
  const int Npad = (N + 63) / 64 * 64;
  std::vector<nbp_fit_plan_req> req;
  for (int fits = 1; fits <= 60; fits++)
    for (int products : {0, 1, 40, 500})
      for (int dim = 1; dim <= 3; dim++)
        for (int kdF : {2, 8})
          for (int g = 0; g < 2; g++) req.push_back({N, fits, fits * dim, products, products ? kdF : 0, g ? 2 * fits + 2 * products : 0});
  std::vector<nbp_fit_plan_rec> rec(req.size());
  if (plan_fits(req.data(), rec.data(), (int64_t)req.size()) != NBP_OK) {
    fprintf(stderr, "nbp_plan_fits failed at N = %d: %s\n", N, last_error());
    exit(2);
  }
  for (const nbp_fit_plan_rec &r : rec) {
    plans++;
    const char *bad = nullptr;
    if (r.status != NBP_OK) bad = "status";
    if (r.threads > 1024 || r.threads != r.P * Npad) bad = "threads";
    if (r.P < 1 || r.P > 4) bad = "P";  // (three rows at Npad = 320: 960 lanes)
    if (r.w5 && !(((Npad / 64) % 4) == 1 && Npad > 64 && r.P == 1 && r.depth == 0)) bad = "w5";
    if (!(r.depth == 0 || r.depth == 2 || r.depth == 3) || r.KS != (r.depth ? (1 << r.depth) - 1 : 1)) bad = "depth / KS";
    // a speculative launch: a rendezvous area per fit, every workgroup that stays resident at once, never inside a round
    if (r.depth && !(r.fits <= SPEC_MAXJOBS && r.coords * r.KS + r.products * r.kdF <= SPEC_MAXBLOCKS && !r.geom_blocks)) bad = "speculation beyond NBP_SPEC_MAXJOBS / NBP_SPEC_MAXBLOCKS";
    // (a plain launch builds no KD tree: the fits' need alone; a prep launch: both)
    if (r.fits > 0 && (size_t)r.lds < nbp_bandwidth_lds_bytes(N, Npad, r.P)) bad = "lds < nbp_bandwidth_lds_bytes";
    if (r.products * r.kdF > 0 && (size_t)r.lds < nbp_kd_lds_bytes(3, N, Npad, r.P)) bad = "lds < nbp_kd_lds_bytes";
    if ((size_t)r.lds > LDS_BYTES) bad = "lds > 160 KB";
    if ((r.prep != 0) != (r.products > 0)) bad = "prep";
    if (bad) {
      failures++;
      if (msgs.size() < 20) {
        char b[384];
        snprintf(b, sizeof(b), "fit plan: %s: N=%d fits=%d coords=%d products=%d kdF=%d geom_blocks=%d -> P=%d depth=%d KS=%d w5=%d threads=%d lds=%ld %s", bad, r.N, r.fits,
                 r.coords, r.products, r.kdF, r.geom_blocks, r.P, r.depth, r.KS, r.w5, r.threads, (long)r.lds, r.kernel);
        msgs.push_back(b);
      }
    }
    sigs.insert(std::make_tuple(std::string(r.kernel), r.P, r.depth, r.w5));
  }
}

static void check_proposals_of(int N, long &plans, long &failures, std::set<std::string> &kernels, std::vector<std::string> &msgs) {
  const int Npad = (N + 63) / 64 * 64;
  std::vector<nbp_proposal_plan_req> req;
  for (int n : {1, 599, 600, 1499, 1500, 3499, 3500, 5000})
    for (int m = 0; m <= 5; m++)
      for (int simple = 0; simple < 2; simple++) req.push_back({N, n, m, simple});
  std::vector<nbp_proposal_plan_rec> rec(req.size());
  if (plan_proposals(req.data(), rec.data(), (int64_t)req.size()) != NBP_OK) exit(2);
  for (const nbp_proposal_plan_rec &r : rec) {
    plans++;
    const char *bad = nullptr;
    // one / two waves per proposal: simple LinearRelative batches on Euclid(2) / Euclid(3) only, rows of at most four / five waves
    if (r.geometry && !(r.simple && (r.manifold == NBP_EUCLID2 || r.manifold == NBP_EUCLID3))) bad = "wave / split geometry for another batch";
    if (r.geometry == 1 && !(N <= (r.manifold == NBP_EUCLID2 ? 256 : 320))) bad = "one wave per proposal beyond its N";
    if (r.geometry == 2 && !(r.manifold == NBP_EUCLID2 && N <= 256)) bad = "two waves per proposal beyond Euclid(2), N <= 256";
    if (r.lds > PROPOSAL_LDS_CAP) bad = "LDS beyond the cap";
    if (r.geometry == 0 && !(r.threads == Npad && r.blocks == r.n)) bad = "workgroup geometry";
    if (r.geometry == 1 && !(r.threads == 64 * NBP_PW_WAVES && (long)r.blocks * NBP_PW_WAVES >= r.n)) bad = "wave geometry";
    if (r.geometry == 2 && !(r.threads == 64 * NBP_PS_W && r.blocks == r.n)) bad = "split geometry";
    if (bad) {
      failures++;
      if (msgs.size() < 20) {
        char b[256];
        snprintf(b, sizeof(b), "proposal plan: %s: N=%d n=%d manifold=%d simple=%d -> geometry=%d blocks=%d threads=%d lds=%ld %s", bad, r.N, r.n, r.manifold, r.simple,
                 r.geometry, r.blocks, r.threads, (long)r.lds, r.kernel);
        msgs.push_back(b);
      }
    }
    kernels.insert(r.kernel);
  }
}

struct option_set { const char *name; const char *var; const char *val; };
static const option_set OPTION_SETS[] = {
    {"defaults", nullptr, nullptr},
    {"NBP_PRODUCT_HL2_MIN=1", "NBP_PRODUCT_HL2_MIN", "1"},
    {"NBP_PRODUCT_NCH=1", "NBP_PRODUCT_NCH", "1"},
    {"NBP_PRODUCT_NCH=8", "NBP_PRODUCT_NCH", "8"},
    {"NBP_PRODUCT_NCH=15", "NBP_PRODUCT_NCH", "15"},
    {"NBP_PRODUCT_ALL_LEVELS_HL=2", "NBP_PRODUCT_ALL_LEVELS_HL", "2"},
    {"NBP_NO_XS_PRODUCTS", "NBP_NO_XS_PRODUCTS", "1"},
    {"NBP_NO_UNIFORM_LATENCY_PRODUCTS", "NBP_NO_UNIFORM_LATENCY_PRODUCTS", "1"},
};
static const option_set FIT_OPTION_SETS[] = {
    {"defaults", nullptr, nullptr},
    {"NBP_NO_SPECULATIVE_FITS", "NBP_NO_SPECULATIVE_FITS", "1"},
    {"NBP_SPEC_DEPTH3=0", "NBP_SPEC_DEPTH3", "0"},
    {"NBP_LCV_P2_MIN=0", "NBP_LCV_P2_MIN", "0"},
    {"NBP_LCV_P1_MIN=0", "NBP_LCV_P1_MIN", "0"},
    {"NBP_NO_W5_FITS", "NBP_NO_W5_FITS", "1"},
};
static const option_set PROPOSAL_OPTION_SETS[] = {
    {"defaults", nullptr, nullptr},
    {"NBP_PROPOSAL_WAVE_MIN=0", "NBP_PROPOSAL_WAVE_MIN", "0"},
    {"NBP_PROPOSAL_SPLIT_MIN=0", "NBP_PROPOSAL_SPLIT_MIN", "0"},
};
static const char *ALL_VARS[] = {"NBP_PRODUCT_HL2_MIN", "NBP_PRODUCT_NCH", "NBP_PRODUCT_ALL_LEVELS_HL", "NBP_NO_XS_PRODUCTS", "NBP_NO_UNIFORM_LATENCY_PRODUCTS",
                                 "NBP_NO_SPECULATIVE_FITS", "NBP_SPEC_DEPTH3", "NBP_LCV_P2_MIN", "NBP_LCV_P1_MIN", "NBP_NO_W5_FITS", "NBP_PROPOSAL_WAVE_MIN",
                                 "NBP_PROPOSAL_SPLIT_MIN"};
static void set_options(const option_set &o) {  // (between the parallel sections: no thread reads the environment meanwhile)
  for (const char *v : ALL_VARS) unsetenv(v);
  if (o.var) setenv(o.var, o.val, 1);
}

// f(N, thread) for every N in 8 .. 512 on `nt` threads
template <class F>
static void for_every_N(int nt, F f) {
  std::atomic<int> next{8};
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      for (int N; (N = next.fetch_add(1)) <= 512;) f(N, t);
    });
  for (std::thread &x : th) x.join();
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s path/to/libnbp.so [rows of the kernel table]\n", argv[0]); return 2; }
  void *h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  plan_products = (plan_products_fn)dlsym(h, "nbp_plan_products");
  plan_fits = (plan_fits_fn)dlsym(h, "nbp_plan_fits");
  plan_proposals = (plan_proposals_fn)dlsym(h, "nbp_plan_proposals");
  last_error = (const char *(*)(void))dlsym(h, "nbp_last_error");
  if (!plan_products || !plan_fits || !plan_proposals || !last_error) { fprintf(stderr, "the library has no plan queries\n"); return 2; }
  const int nrows = argc > 2 ? atoi(argv[2]) : 25;
  unsigned hw = std::thread::hardware_concurrency();
  const int nt = hw == 0 ? 4 : (hw > 16 ? 16 : (int)hw);
  long failures = 0;
  tally all;
  for (const option_set &o : OPTION_SETS) {
    set_options(o);
    std::vector<tally> per(nt);
    for_every_N(nt, [&](int N, int t) { check_products_of(N, per[t]); });
    tally sum;
    for (const tally &p : per) sum.merge(p);
    printf("products [%s]: %ld plans, %ld launched, %zu signatures, %zu rows, refused: %ld big-in-round %ld lds %ld no-kernel, %ld not a launch's arguments, %ld sizing queries, %ld oversize, %ld failures\n",
           o.name, sum.plans, sum.ok, sum.sigs.size(), sum.rows.size(), sum.refused[1], sum.refused[2], sum.refused[3], sum.invalid, sum.sizing, sum.oversize, sum.failures);
    if (!o.var && (int)sum.rows.size() != nrows) {
      printf("FAIL: the default options reach %zu of the %d rows of the kernel table\n", sum.rows.size(), nrows);
      failures++;
    }
    all.merge(sum);
  }
  for (const std::string &m : all.msgs) printf("FAIL: %s\n", m.c_str());
  for (const std::string &m : all.over_msgs) printf("OVERSIZE: %s\n", m.c_str());
  failures += all.failures;
  printf("products total: %ld plans checked, %ld launched, %zu distinct signatures, %ld refusals, %ld oversize\n", all.plans, all.ok, all.sigs.size(),
         all.refused[1] + all.refused[2] + all.refused[3], all.oversize);

  long fplans = 0, ffail = 0;
  std::set<std::tuple<std::string, int, int, int>> fsigs;
  std::vector<std::string> fmsgs;
  std::mutex mu;
  for (const option_set &o : FIT_OPTION_SETS) {
    set_options(o);
    for_every_N(nt, [&](int N, int) {
      long p = 0, f = 0;
      std::set<std::tuple<std::string, int, int, int>> s;
      std::vector<std::string> m;
      check_fits_of(N, p, f, s, m);
      std::lock_guard<std::mutex> g(mu);
      fplans += p; ffail += f;
      fsigs.insert(s.begin(), s.end());
      for (const std::string &x : m) if (fmsgs.size() < 20) fmsgs.push_back(x);
    });
  }
  for (const std::string &m : fmsgs) printf("FAIL: %s\n", m.c_str());
  printf("fits total: %ld plans checked, %zu distinct signatures, %ld failures\n", fplans, fsigs.size(), ffail);

  long pplans = 0, pfail = 0;
  std::set<std::string> pk;
  std::vector<std::string> pmsgs;
  for (const option_set &o : PROPOSAL_OPTION_SETS) {
    set_options(o);
    for (int N = 8; N <= 512; N++) check_proposals_of(N, pplans, pfail, pk, pmsgs);
  }
  for (const std::string &m : pmsgs) printf("FAIL: %s\n", m.c_str());
  printf("proposals total: %ld plans checked, %zu kernels, %ld failures\n", pplans, pk.size(), pfail);
  set_options(OPTION_SETS[0]);
  failures += ffail + pfail;
  printf("%s: %ld failures, %ld oversize plans\n", failures ? "FAILED" : "ok", failures, all.oversize);
  return failures ? 1 : 0;
}
