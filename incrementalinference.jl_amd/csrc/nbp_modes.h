// nbp_modes.h -- the modes of resident beliefs: mean-shift over a belief's own KDE from every one of its points, the end points
// merged into modes and the modes ranked, all in one launch.  DESIGN.md 3 ("Modes of a belief") holds the definition:
//   g_d       = bw_scale h_d, r_d = 1 / g_d
//   ascent    y <- x_i; w_j = exp(e(y, x_j)), e the exponent of nbp_kde.h over all D coordinates with r; S = sum_j w_j;
//             m_d = sum_j w_j delta_d(x_j, y) (wrapped on circular coordinates); y_d <- y_d + m_d / S (wrapped likewise);
//             j = 0 .. c - 1 in that order in one lane, one rounding per written operation: the trajectory of a start depends on
//             the belief and the options alone, not on the beliefs that share the launch
//   stop      after the first iteration with max_d |m_d / S| / g_d <= tol (converged), or after max_iter iterations
//   merging   leader clustering in index order: the lowest unassigned i leads, every unassigned k > i with
//             max_d |delta_d(y_k, y_i)| / g_d <= merge joins it
//   ranking   by member count descending, equal counts by the lower leader index
//   density   S at the leader's end point / kde_norm(c, g)
// S never vanishes: a start is a point of the belief, so its own term makes S >= 1 at the first iteration, and a mean-shift step
// does not decrease the density S / norm (with a Gaussian kernel the step maximises a lower bound of it that is tight at y).
// (Independently of that, exp_nonpos clamps its argument at -700: every w_j is a positive number.)
// A bandwidth entry h_d or g_d that is not a positive finite number: n_modes = 0, labels -1, every record empty.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"


// the sums of one mean-shift step at y over the rows of X[3][N] in LDS (every lane of a wave reads the same address: broadcast)
__device__ __forceinline__ void modes_sums(double y0, double y1, double y2, const double *X, int N, int c, bool k1, bool k2, bool c0,
                                           bool c2, double r0, double r1, double r2, const double *tab, double &S, double &m0,
                                           double &m1, double &m2) {
  S = 0.0;
  m0 = 0.0;
  m1 = 0.0;
  m2 = 0.0;
  for (int j = 0; j < c; j++) {
    const double w = exp_nonpos(kde_exponent(y0, y1, y2, X, N, j, true, k1, k2, c0, c2, r0, r1, r2), tab);
    S += w;
    double d0 = X[j] - y0;
    if (c0) d0 = wrap_pi(d0);
    m0 += w * d0;
    if (k1) m1 += w * (X[N + j] - y1);
    if (k2) {
      double d2 = X[2 * N + j] - y2;
      if (c2) d2 = wrap_pi(d2);
      m2 += w * d2;
    }
  }
}

// max_d |delta_d| / g_d of a step or of the difference of two end points (already wrapped)
__device__ __forceinline__ double modes_reach(double d0, double d1, double d2, bool k1, bool k2, double g0, double g1, double g2) {
  double q = fabs(d0) / g0;
  if (k1) q = fmax(q, fabs(d1) / g1);
  if (k2) q = fmax(q, fabs(d2) / g2);
  return q;
}

// hdr: (n_modes, n_unconverged) per belief; labels, iters: N per belief; recs: NBP_MODES_MAX per belief
#define NBP_MODES_ARGS                                                                                                           \
  const int32_t *slots, const int32_t *manifolds, const double *arena, int N, int64_t S, nbp_modes_opts o, nbp_mode_rec *recs, \
      int32_t *hdr, int32_t *labels, int32_t *iters
#if NBP_TU & NBP_TU_MODES
// One workgroup per belief, 64 ceil(N / 64) lanes (nbp_ppe_kernel's shape).  LDS: exp table | X[3][N] | Y[3][N] | red | lab[N] |
// cnt[N] | rnk[N].  Lane i owns start i; a wave iterates until all of its starts have stopped (N^2 D operations per iteration and
// belief).  The merging walks the leaders in index order: a ballot per wave and a minimum over the waves find the lowest unassigned
// lane, one compare in every lane joins its members (one barrier per leader: the per-wave minima alternate between two halves of
// `red`).  The workgroup counts the members (integer LDS atomics) and ranks its leaders.  The manifold is a runtime value.
__global__ void __launch_bounds__(512)
nbp_modes_kernel(NBP_MODES_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *X = smem + NBP_EXPTAB, *Y = X + 3 * N, *red = Y + 3 * N;
  int *redi = (int *)red, *lab = (int *)(red + NBP_RED), *cnt = lab + N, *rnk = cnt + N;
  const int b = blockIdx.x, n = threadIdx.x, lane = n & 63, wv = n >> 6, nw = (blockDim.x + 63) >> 6;
  const double *s = arena + S * slots[b];
  const int M = manifolds[b], D = mani_dim(M);
  const int c = slot_count(s, N);
  nbp_exp_tab_init(tab);
  if (n < c)
    for (int k = 0; k < D; k++) X[k * N + n] = s[k * N + n];
  if (n < N) cnt[n] = 0;
  __syncthreads();
  const bool k1 = D > 1, k2 = D > 2, c0 = is_circ(M, 0), c2 = is_circ(M, 2);
  const double h0 = s[3 * N], h1 = k1 ? s[3 * N + 1] : 1.0, h2 = k2 ? s[3 * N + 2] : 1.0;
  const double g0 = o.bw_scale * h0, g1 = o.bw_scale * h1, g2 = o.bw_scale * h2;
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1) & kde_bw_ok(h2) & kde_bw_ok(g0) & kde_bw_ok(g1) & kde_bw_ok(g2);  // block-uniform
  const double r0 = 1.0 / g0, r1 = 1.0 / g1, r2 = 1.0 / g2;
  const bool mine = valid && n < c;
  // (three scalars: an array indexed by the loop lives in scratch)
  double y0 = mine ? X[n] : 0.0, y1 = (mine && k1) ? X[N + n] : 0.0, y2 = (mine && k2) ? X[2 * N + n] : 0.0;

  // ---- ascent ----
  bool active = mine, conv = false;
  int it = 0;
  while (__builtin_amdgcn_ballot_w64(active) != 0) {  // (the lanes that have stopped ride along: their sums are not used)
    double Sw, m0, m1, m2;
    modes_sums(y0, y1, y2, X, N, c, k1, k2, c0, c2, r0, r1, r2, tab, Sw, m0, m1, m2);
    if (active) {
      const double s0 = m0 / Sw, s1 = k1 ? m1 / Sw : 0.0, s2 = k2 ? m2 / Sw : 0.0;
      y0 = y0 + s0;
      if (c0) y0 = wrap_pi(y0);
      y1 = y1 + s1;
      y2 = y2 + s2;
      if (c2) y2 = wrap_pi(y2);
      it++;
      conv = modes_reach(s0, s1, s2, k1, k2, g0, g1, g2) <= o.tol;
      active = !conv && it < o.max_iter;
    }
  }
  if (n < N) {
    Y[n] = y0;
    Y[N + n] = y1;
    Y[2 * N + n] = y2;
  }
  {
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(mine && !conv);
    if (lane == 0) redi[32 + wv] = __popcll(bal);
  }
  __syncthreads();  // Y and the counts of the unconverged are written

  // ---- merging: leaders in index order ----
  int leader = -1;
  bool un = mine;
  for (int step = 0;; step++) {
    int *buf = redi + (step & 1) * 16;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(un);
    if (lane == 0) buf[wv] = bal ? (wv << 6) + (int)__builtin_ctzll(bal) : 0x7fffffff;
    __syncthreads();
    int lead = 0x7fffffff;
    for (int q = 0; q < nw; q++) lead = min(lead, buf[q]);
    if (lead == 0x7fffffff) break;  // block-uniform: every lane reads the same minima
    if (un) {                       // (an unassigned lane has n >= lead)
      bool join = n == lead;
      if (!join) {
        double d0 = y0 - Y[lead], d2 = y2 - Y[2 * N + lead];
        const double d1 = y1 - Y[N + lead];
        if (c0) d0 = wrap_pi(d0);
        if (c2) d2 = wrap_pi(d2);
        join = modes_reach(d0, d1, d2, k1, k2, g0, g1, g2) <= o.merge;
      }
      if (join) {
        leader = lead;
        un = false;
      }
    }
  }
  if (leader >= 0) atomicAdd(&cnt[leader], 1);
  if (n < N) lab[n] = leader;
  __syncthreads();

  // ---- ranking: by count descending, equal counts by the lower leader index ----
  const bool leads = leader == n;  // (n < c: leader >= 0 only there)
  int rank = 0;
  if (leads) {
    const int own = cnt[n];
    for (int j = 0; j < c; j++) {
      const int cj = cnt[j];
      if (lab[j] == j && (cj > own || (cj == own && j < n))) rank++;
    }
    rnk[n] = rank;
  }
  {
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(leads);
    if (lane == 0) redi[48 + wv] = __popcll(bal);
  }
  __syncthreads();
  int n_modes = 0, n_unconv = 0;
  for (int q = 0; q < nw; q++) {
    n_modes += redi[48 + q];
    n_unconv += redi[32 + q];
  }

  // ---- output ----
  if (n < N) {
    labels[(size_t)b * N + n] = leader >= 0 ? rnk[leader] : -1;
    iters[(size_t)b * N + n] = it;
  }
  nbp_mode_rec *rec = recs + (size_t)b * NBP_MODES_MAX;
  if (leads && rank < NBP_MODES_MAX) {
    double Sw, m0, m1, m2;
    modes_sums(y0, y1, y2, X, N, c, k1, k2, c0, c2, r0, r1, r2, tab, Sw, m0, m1, m2);
    nbp_mode_rec *r = rec + rank;
    r->location[0] = y0;
    r->location[1] = y1;
    r->location[2] = y2;
    r->density = Sw / kde_norm(c, true, k1, k2, g0, g1, g2);
    r->count = cnt[n];
    r->leader = n;
  }
  if (n < NBP_MODES_MAX && n >= n_modes) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    nbp_mode_rec *r = rec + n;
    r->location[0] = nan;
    r->location[1] = k1 ? nan : 0.0;
    r->location[2] = k2 ? nan : 0.0;
    r->density = nan;
    r->count = 0;
    r->leader = -1;
  }
  if (n == 0) {
    hdr[2 * b] = n_modes;
    hdr[2 * b + 1] = n_unconv;
  }
}
#else
__global__ void nbp_modes_kernel(NBP_MODES_ARGS);
#endif

static inline size_t nbp_modes_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 6 * (size_t)N + NBP_RED) * 8 + 3 * (size_t)N * 4; }
