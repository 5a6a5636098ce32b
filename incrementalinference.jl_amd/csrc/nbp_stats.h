// nbp_stats.h -- the spread of a resident belief and how far one belief lies from another: calcMeanCovar
// (services/VariableStatistics.jl:39-44; Statistics.cov(vartype, pts), VariableStatistics.jl:12-19) and kld(p, q)
// (attic/examples/FixedPointIllustrationsSquare.jl:53-62).  DESIGN.md 3, "Belief statistics", holds the definitions; coordinates are
// tangent coordinates at the identity (Euclid(1-3); the circle; SE(2): x, y, theta), c the count a slot holds, D the dimension.
//   mean[d]    = mean_geodesic_coord in the workgroup shape nbp_ppe_kernel calls it in: the bits of nbp_run_ppe's mean of the slot
//   delta[i][d] = x[i][d] - mean[d], wrapped to [-pi, pi) on circular coordinates (stats_deviation: the ONE place it is formed)
//   cov[d][e]  = (1 / (c - 1)) sum_{i < c} delta[i][d] delta[i][e]; each of the D (D + 1) / 2 sums is formed once (lane i adds
//                point i, block_sum), the other triangle is the same double copied.  NBP_MAXD x NBP_MAXD doubles per belief,
//                row-major, rows and columns beyond D zero.  c < 2: the D x D block is NaN (Julia's corrected covariance of one
//                observation); the mean is delivered all the same.  The bandwidth plays no part.
//   SE(2): the deviations are taken in the world frame about the mean, heading wrapped -- not the Lie-algebra coordinates at the
//                mean of Manifolds.jl's cov(M, pts; basis).  DEFINED here, unpinned.
//   l_p(x)     = M + log(sum_{j < m} exp(e_j - M)) - log(norm) for a belief p of m points y_j and bandwidth h, e_j = e(x, y_j) and
//                norm the exponent and the normalisation of nbp_kde.h, M = max_j e_j; j = 0 .. m - 1 in that order in one lane (two
//                passes: the maximum, then the sum).  The logarithm of the density nbp_run_evaluate defines, finite where that density
//                underflows to zero.
//   kld(a, b)  = Eaa - Eab, Eaa = (1 / n) sum_{i < n} l_a(a_i) (the self term stays in), Eab = (1 / n) sum_{i < n} l_b(a_i); both
//                means in one summation order (lane i, block_sum), both l from one device function: a belief against a
//                bit-identical copy, or against its own slot, gives exactly 0.0.  No clamp at zero; entropy(a) = -Eaa.  A bandwidth
//                entry of either belief that is not a positive finite number: kld and both terms are NaN.  This form is restated
//                from memory of KernelDensityEstimate.jl's direct kld and is unpinned.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"


// one record per belief; entries beyond the manifold's dimension are zero
struct nbp_meancov_rec {
  double mean[NBP_MAXD];
  double cov[NBP_MAXD * NBP_MAXD];
};
// one record per pair
struct nbp_kld_rec {
  double kld, eaa, eab;
};

#define NBP_MEANCOV_ARGS const int32_t *slots, const int32_t *manifolds, const double *arena, int N, int64_t S, nbp_meancov_rec *out
#define NBP_KLD_ARGS                                                                                                   \
  const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, const double *arena, int N, int64_t S,     \
      nbp_kld_rec *out
#if NBP_TU & (NBP_TU_STATS | NBP_TU_CREDIBLE | NBP_TU_MIXTURE)
// the deviation of a coordinate from the mean: the world frame, circular coordinates wrapped.  (Pinning SE(2) to Manifolds.jl's
// coordinates at the mean would change this function alone.)
__device__ __forceinline__ double stats_deviation(double x, double mu, bool circ) {
  const double d = x - mu;
  return circ ? wrap_pi(d) : d;
}
#endif

#if NBP_TU & NBP_TU_STATS

// One workgroup per belief, 64 ceil(N / 64) lanes (the shape of nbp_ppe_kernel: the mean's bits depend on it).  LDS: X[3][N] | red.
// Lane i owns point i; six block_sums at most.  The manifold is a runtime value.  No atomics.
__global__ void __launch_bounds__(512)
nbp_meancov_kernel(NBP_MEANCOV_ARGS) {
  extern __shared__ double smem[];
  double *X = smem, *red = X + 3 * N;
  const double *s = arena + S * slots[blockIdx.x];
  const int M = manifolds[blockIdx.x], D = mani_dim(M), n = threadIdx.x;
  const int c = slot_count(s, N);
  if (n < c)
    for (int k = 0; k < D; k++) X[k * N + n] = s[k * N + n];
  __syncthreads();
  // (scalars, as in nbp_ppe_kernel: an array indexed by a loop lives in scratch)
  const double mu0 = mean_geodesic_coord(X, c, M, 0, red);
  const double mu1 = D > 1 ? mean_geodesic_coord(X + N, c, M, 1, red) : 0.0;
  const double mu2 = D > 2 ? mean_geodesic_coord(X + 2 * N, c, M, 2, red) : 0.0;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  if (n < c) {
    d0 = stats_deviation(X[n], mu0, is_circ(M, 0));
    if (D > 1) d1 = stats_deviation(X[N + n], mu1, false);
    if (D > 2) d2 = stats_deviation(X[2 * N + n], mu2, is_circ(M, 2));
  }
  const double s00 = block_sum(d0 * d0, red);
  double s01 = 0.0, s11 = 0.0, s02 = 0.0, s12 = 0.0, s22 = 0.0;
  if (D > 1) {  // (block-uniform)
    s01 = block_sum(d0 * d1, red);
    s11 = block_sum(d1 * d1, red);
  }
  if (D > 2) {
    s02 = block_sum(d0 * d2, red);
    s12 = block_sum(d1 * d2, red);
    s22 = block_sum(d2 * d2, red);
  }
  if (n == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double den = (double)(c - 1);
    const bool ok = c >= 2;
    nbp_meancov_rec *r = out + blockIdx.x;
    r->mean[0] = mu0;
    r->mean[1] = mu1;
    r->mean[2] = mu2;
    const double c00 = ok ? s00 / den : nan;
    const double c01 = D > 1 ? (ok ? s01 / den : nan) : 0.0, c11 = D > 1 ? (ok ? s11 / den : nan) : 0.0;
    const double c02 = D > 2 ? (ok ? s02 / den : nan) : 0.0, c12 = D > 2 ? (ok ? s12 / den : nan) : 0.0;
    const double c22 = D > 2 ? (ok ? s22 / den : nan) : 0.0;
    r->cov[0] = c00;
    r->cov[1] = c01;
    r->cov[2] = c02;
    r->cov[3] = c01;
    r->cov[4] = c11;
    r->cov[5] = c12;
    r->cov[6] = c02;
    r->cov[7] = c12;
    r->cov[8] = c22;
  }
}

// l_p(x): the one function, and the one order, behind Eaa and Eab.  cnt >= 1; h positive and finite (the caller has checked).
__device__ __forceinline__ double stats_log_density(double x0, double x1, double x2, const double *Y, int N, int cnt, int D, bool c0,
                                                    bool c2, double h0, double h1, double h2, const double *tab) {
  const double r0 = 1.0 / h0, r1 = 1.0 / h1, r2 = 1.0 / h2;
  const bool k1 = D > 1, k2 = D > 2;
  double mx = -INFINITY;
  for (int j = 0; j < cnt; j++) mx = fmax(mx, kde_exponent(x0, x1, x2, Y, N, j, true, k1, k2, c0, c2, r0, r1, r2));
  double acc = 0.0;
  for (int j = 0; j < cnt; j++) acc += exp_nonpos(kde_exponent(x0, x1, x2, Y, N, j, true, k1, k2, c0, c2, r0, r1, r2) - mx, tab);
  const double norm = kde_norm(cnt, true, k1, k2, h0, h1, h2);
  return mx + nbpm_log(acc) - nbpm_log(norm);
}

// One workgroup per pair of slots, 64 ceil(N / 64) lanes (at most 512).  LDS: exp table | A[3][N] | B[3][N] | red.  Lane i owns a_i
// and walks j over a's rows and over b's rows (every lane of a wave reads the same address: broadcast reads), twice each: the
// maximum, then the sum.  block_sum adds the lanes; lane 0 writes the record.  A value depends on the pair alone.  No atomics.
__global__ void __launch_bounds__(512)
nbp_kld_kernel(NBP_KLD_ARGS) {
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
  const double ha0 = sa[3 * N], ha1 = D > 1 ? sa[3 * N + 1] : 1.0, ha2 = D > 2 ? sa[3 * N + 2] : 1.0;
  const double hb0 = sb[3 * N], hb1 = D > 1 ? sb[3 * N + 1] : 1.0, hb2 = D > 2 ? sb[3 * N + 2] : 1.0;
  const bool valid = kde_bw_ok(ha0) & kde_bw_ok(ha1) & kde_bw_ok(ha2) & kde_bw_ok(hb0) & kde_bw_ok(hb1) & kde_bw_ok(hb2);  // block-uniform
  double la = 0.0, lb = 0.0;
  if (valid && n < ca) {
    const bool c0 = is_circ(M, 0), c2 = is_circ(M, 2);
    const double x0 = A[n], x1 = D > 1 ? A[N + n] : 0.0, x2 = D > 2 ? A[2 * N + n] : 0.0;
    la = stats_log_density(x0, x1, x2, A, N, ca, D, c0, c2, ha0, ha1, ha2, tab);
    lb = stats_log_density(x0, x1, x2, B, N, cb, D, c0, c2, hb0, hb1, hb2, tab);
  }
  const double sum_a = block_sum(la, red), sum_b = block_sum(lb, red);
  if (n == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double eaa = valid ? sum_a / (double)ca : nan, eab = valid ? sum_b / (double)ca : nan;
    nbp_kld_rec *r = out + blockIdx.x;
    r->kld = eaa - eab;
    r->eaa = eaa;
    r->eab = eab;
  }
}
#else
__global__ void nbp_meancov_kernel(NBP_MEANCOV_ARGS);
__global__ void nbp_kld_kernel(NBP_KLD_ARGS);
#endif

static inline size_t nbp_meancov_lds_bytes(int N) { return (3 * (size_t)N + NBP_RED) * 8; }
static inline size_t nbp_kld_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 6 * (size_t)N + NBP_RED) * 8; }
