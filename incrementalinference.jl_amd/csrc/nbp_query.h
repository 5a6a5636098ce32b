// nbp_query.h -- what a caller asks of a resident belief besides its points and its point estimate: the density of its KDE at
// query points (the reference's `getBelief(fg, :x0)([l0])`) and the distance between two beliefs (`mmd(p1, p2, varType; bw)`,
// services/SolverUtilities.jl:25-47).  DESIGN.md 3 holds the definitions; coordinates are tangent coordinates at the identity
// (SE(2): x, y, theta), as in nbp_ppe.h.
//   density  p(q) = 1 / norm * sum_{j < c} exp(e(q, x_j)), e and norm the exponent and the normalisation of nbp_kde.h; j = 0 ..
//            c - 1 in that order in ONE lane per query, so a value depends neither on the launch geometry nor on the queries that
//            travel with it.  The PPE's p_i (nbp_ppe.h) with the normalisation added: exact on Euclidean coordinates; on a
//            circular coordinate the mass a kernel has beyond +-pi is lost.  All D coordinates enter (partial beliefs are not
//            treated specially; the marginal of nbp_marginal.h is this body with a coordinate mask).  A bandwidth entry that is
//            not a positive finite number: every density of that belief is NaN.  (A term below exp(-700) enters as ~1e-304, the
//            clamp of exp_nonpos, not as 0.)
//   mmd      k(p, q) = exp(-sigma d(p, q)^2), d^2 = sum_d w_d delta_d^2 (circular coordinates wrapped; w_d = 1 but for the heading
//            of SE(2), NBP_MMD_SE2_HEADING_WEIGHT), S_xy = sum_i sum_j k(x_i, y_j),
//            mmd = Saa / (n n) + Sbb / (m m) - 2 Sab / (n m), evaluated as written; the beliefs' bandwidths play no part.  All
//            three sums come from one device function in one order (lane i adds j = 0 .. count - 1, block_sum over i): the mmd
//            of a belief with a bit-identical copy of itself is exactly 0.0.  No clamp at zero.
// Both are DEFINED here and unpinned against KernelDensityEstimate.jl / ApproxManifoldProducts.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"


#define NBP_QUERY_TILE 256  // queries of one belief per workgroup of nbp_eval_kernel: one lane each
// Weight of the squared heading difference in the mmd's squared distance on SE(2).  Manifolds.jl's Frobenius metric on the
// rotation part would make it 2; AMP's `ker` is restated from memory, and until it is pinned the weight is 1.
#define NBP_MMD_SE2_HEADING_WEIGHT 1.0

// nbp_eval_kernel -- tiles: (belief b of the batch, first query, number of queries <= NBP_QUERY_TILE), three ints each, built by the
// host; queries: NBP_MAXD doubles each, all beliefs' back to back; dens: one double per query.
#define NBP_EVAL_ARGS                                                                                                  \
  const int32_t *tiles, const int32_t *slots, const int32_t *manifolds, const double *arena, int N, int64_t S,         \
      const double *queries, double *dens
#define NBP_MMD_ARGS                                                                                                   \
  const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, const double *arena, int N, int64_t S,     \
      double sigma, double *out
#if NBP_TU & (NBP_TU_QUERY | NBP_TU_MARGINAL)
// The body of both point-density kernels.  One workgroup per tile, NBP_QUERY_TILE lanes.  LDS: exp table | X[3][N].  Lane t owns
// query t of the tile and walks j over the LDS rows (every lane reads the same address: broadcast reads); c D operations per query,
// no atomics, no reduction.  K: the bit mask of the coordinates that enter (block-uniform; bits beyond the manifold's dimension are
// not looked at).  The bandwidth and the query of a coordinate outside K are not read.
__device__ __forceinline__ void eval_body(NBP_EVAL_ARGS, const int K) {
  extern __shared__ double smem[];
  double *tab = smem, *X = smem + NBP_EXPTAB;
  const int b = tiles[3 * blockIdx.x], q0 = tiles[3 * blockIdx.x + 1], nq = tiles[3 * blockIdx.x + 2];
  const double *s = arena + S * slots[b];
  const int M = manifolds[b], D = mani_dim(M), t = threadIdx.x;
  const bool k0 = K & 1, k1 = D > 1 && (K & 2), k2 = D > 2 && (K & 4);
  const int c = slot_count(s, N);
  nbp_exp_tab_init(tab);
  for (int i = t; i < c; i += blockDim.x)
    for (int k = 0; k < D; k++) X[k * N + i] = s[k * N + i];
  __syncthreads();
  const double h0 = k0 ? s[3 * N] : 1.0, h1 = k1 ? s[3 * N + 1] : 1.0, h2 = k2 ? s[3 * N + 2] : 1.0;
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1) & kde_bw_ok(h2);
  if (t >= nq) return;
  double p = __longlong_as_double(0x7ff8000000000000ll);
  if (valid) {
    const double *q = queries + (size_t)NBP_MAXD * (size_t)(q0 + t);
    const double r0 = 1.0 / h0, r1 = 1.0 / h1, r2 = 1.0 / h2;
    const bool c0 = is_circ(M, 0), c2 = is_circ(M, 2);
    const double x0 = k0 ? q[0] : 0.0, x1 = k1 ? q[1] : 0.0, x2 = k2 ? q[2] : 0.0;
    p = 0.0;
    for (int j = 0; j < c; j++) p += exp_nonpos(kde_exponent(x0, x1, x2, X, N, j, k0, k1, k2, c0, c2, r0, r1, r2), tab);
    p /= kde_norm(c, k0, k1, k2, h0, h1, h2);
  }
  dens[q0 + t] = p;
}
#endif

#if NBP_TU & NBP_TU_QUERY
__global__ void __launch_bounds__(NBP_QUERY_TILE)
nbp_eval_kernel(NBP_EVAL_ARGS) {
  eval_body(tiles, slots, manifolds, arena, N, S, queries, dens, 7);
}

// sum_{j < cnt} k(x, y_j): the one function, and the one order, behind Saa, Sab and Sbb
__device__ __forceinline__ double mmd_row_sum(double x0, double x1, double x2, const double *Y, int N, int cnt, int D, bool c0,
                                              bool c2, double sigma, const double *tab) {
  const double w2 = c2 ? NBP_MMD_SE2_HEADING_WEIGHT : 1.0;
  double acc = 0.0;
  for (int j = 0; j < cnt; j++) {
    double d0 = x0 - Y[j];
    if (c0) d0 = wrap_pi(d0);
    double e = d0 * d0;
    if (D > 1) {
      const double d1 = x1 - Y[N + j];
      e += d1 * d1;
    }
    if (D > 2) {
      double d2 = x2 - Y[2 * N + j];
      if (c2) d2 = wrap_pi(d2);
      e += w2 * d2 * d2;
    }
    acc += exp_nonpos(-sigma * e, tab);
  }
  return acc;
}

// One workgroup per pair of slots, 64 ceil(N / 64) lanes.  LDS: exp table | A[3][N] | B[3][N] | red.  Lane i owns a_i and b_i and
// forms its rows of Saa, Sab and Sbb; block_sum adds the lanes; lane 0 writes the value.  No atomics.
__global__ void __launch_bounds__(512)
nbp_mmd_kernel(NBP_MMD_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *A = smem + NBP_EXPTAB, *B = A + 3 * N, *red = B + 3 * N;
  const double *sa = arena + S * slots_a[blockIdx.x], *sb = arena + S * slots_b[blockIdx.x];
  const int M = manifolds[blockIdx.x], D = mani_dim(M), n = threadIdx.x;
  const int ca = slot_count(sa, N), cb = slot_count(sb, N);
  nbp_exp_tab_init(tab);
  for (int k = 0; k < D; k++) {
    if (n < ca) A[k * N + n] = sa[k * N + n];
    if (n < cb) B[k * N + n] = sb[k * N + n];
  }
  __syncthreads();
  const bool c0 = is_circ(M, 0), c2 = is_circ(M, 2);
  double raa = 0.0, rab = 0.0, rbb = 0.0;
  if (n < ca) {
    const double x0 = A[n], x1 = D > 1 ? A[N + n] : 0.0, x2 = D > 2 ? A[2 * N + n] : 0.0;
    raa = mmd_row_sum(x0, x1, x2, A, N, ca, D, c0, c2, sigma, tab);
    rab = mmd_row_sum(x0, x1, x2, B, N, cb, D, c0, c2, sigma, tab);
  }
  if (n < cb) {
    const double x0 = B[n], x1 = D > 1 ? B[N + n] : 0.0, x2 = D > 2 ? B[2 * N + n] : 0.0;
    rbb = mmd_row_sum(x0, x1, x2, B, N, cb, D, c0, c2, sigma, tab);
  }
  const double saa = block_sum(raa, red), sab = block_sum(rab, red), sbb = block_sum(rbb, red);
  if (n == 0) {
    const double na = (double)ca, nb = (double)cb;
    out[blockIdx.x] = saa / (na * na) + sbb / (nb * nb) - 2.0 * sab / (na * nb);
  }
}
#else
__global__ void nbp_eval_kernel(NBP_EVAL_ARGS);
__global__ void nbp_mmd_kernel(NBP_MMD_ARGS);
#endif

static inline size_t nbp_eval_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 3 * (size_t)N) * 8; }
static inline size_t nbp_mmd_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 6 * (size_t)N + NBP_RED) * 8; }
