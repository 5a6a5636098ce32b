// nbp_credible.h -- how much of a resident belief lies where: the levels of its highest-density regions, the credibility of
// reference points (is the ground truth inside the 90 % region?) and the quantiles of its coordinates.  DESIGN.md 3, "Credible
// regions", holds the definitions; include/nbp.h states them at nbp_run_credible.  Coordinates are tangent coordinates at the
// identity (Euclid(1-3); the circle; SE(2): x, y, theta), c the count a slot holds, K the coordinate mask (bit d = coordinate d).
//   l_i       = M_i + log(sum_{j != i} exp(e_ij - M_i)) - log((c - 1) prod_{d in K} sqrt(2 pi) h_d): the leave-one-out log density of
//               own point i, e and the normalisation those of nbp_kde.h on K, j ascending in one lane, two passes (the maximum, then
//               the sum).  Exclusion is by index.  With nothing left out and the full mask this is stats_log_density's sequence of
//               operations (nbp_stats.h): that form serves the queries.
//   order     = the indices by ascending (l_i, i); level(a) = l at position c - ceil(a c) of that order; n_inside by binary search.
//   query q   : l_q over all c points, n_above = #{i : l_i > l_q} by binary search in the sorted l, mass = n_above / c.
//   quantiles : per coordinate of the manifold, the sorted x_id (circular: stats_deviation about the mean, the result wrapped back),
//               type 7.  The bandwidth plays no part.
// DEFINED here, unpinned.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"
#include "nbp_stats.h"  // stats_deviation

// the sort's length: the next power of two >= N, at least one wave (N <= 512: at most 512)
__host__ __device__ static inline int nbp_credible_P(int N) {
  int P = 64;
  while (P < N) P <<= 1;
  return P;
}

#define NBP_CREDIBLE_ARGS                                                                                              \
  const int32_t *slots, const int32_t *manifolds, const int32_t *masks, const nbp_credible_opts *opts,                 \
      const int32_t *q_first, const double *queries, const double *arena, int N, int64_t S, nbp_credible_rec *rec,     \
      double *logdens, int32_t *order, nbp_credibility_rec *qrec
#if NBP_TU & NBP_TU_CREDIBLE
// l_p(x) on the masked coordinates with point `skip` of the belief left out (skip < 0: nothing left out).  cnt - (skip >= 0) >= 1; the
// bandwidth entries that enter are positive and finite (the caller has checked).  A point that is left out adds +0.0 to the sum.
__device__ __forceinline__ double cred_log_density(double x0, double x1, double x2, const double *Y, int N, int cnt, int skip, bool k0,
                                                   bool k1, bool k2, bool c0, bool c2, double h0, double h1, double h2,
                                                   const double *tab) {
  const double r0 = 1.0 / h0, r1 = 1.0 / h1, r2 = 1.0 / h2;
  double mx = -INFINITY;
  for (int j = 0; j < cnt; j++) {
    const double e = kde_exponent(x0, x1, x2, Y, N, j, k0, k1, k2, c0, c2, r0, r1, r2);
    mx = j == skip ? mx : fmax(mx, e);
  }
  double acc = 0.0;
  for (int j = 0; j < cnt; j++) {
    const double w = exp_nonpos(kde_exponent(x0, x1, x2, Y, N, j, k0, k1, k2, c0, c2, r0, r1, r2) - mx, tab);
    acc += j == skip ? 0.0 : w;
  }
  const double norm = kde_norm(skip < 0 ? cnt : cnt - 1, k0, k1, k2, h0, h1, h2);
  return mx + nbpm_log(acc) - nbpm_log(norm);
}

// Bitonic sort of P (value, index) pairs in LDS, ascending, compared lexicographically: the indices are distinct, so the result does
// not depend on the network.  P a power of two, blockDim.x >= P / 2: one compare-exchange per lane per step, a barrier between steps
// (45 steps at P = 512).  Every lane of the workgroup calls.  (A NaN value compares false both ways: nothing is lost, nothing is
// read out of bounds, the order is then unspecified.)
__device__ __forceinline__ void cred_sort(double *key, int32_t *idx, int P) {
  const int t = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      if (t < (P >> 1)) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const double ka = key[lo], kb = key[hi];
        const int32_t ia = idx[lo], ib = idx[hi];
        const bool after = ka > kb || (ka == kb && ia > ib);
        if (after == up) {
          key[lo] = kb;
          key[hi] = ka;
          idx[lo] = ib;
          idx[hi] = ia;
        }
      }
    }
  __syncthreads();
}
// the first position of the ascending key[0 .. c) whose value is >= v (strict: > v); c where there is none
__device__ __forceinline__ int cred_first_at_or_above(const double *key, int c, double v, bool strict) {
  int lo = 0, hi = c;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (strict ? key[m] <= v : key[m] < v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// One workgroup per belief, 64 ceil(N / 64) lanes (the shape of nbp_meancov_kernel: the mean's bits depend on it).
// LDS: exp table | X[3][N] | key[P] | idx[P] (int32) | red, P = nbp_credible_P(N).  Lane i owns point i: it walks j over the LDS rows
// twice (every lane of a wave reads the same address: broadcast reads) for l_i; the (l_i, i) pairs are sorted in LDS and stay there
// for the levels and the queries (one query per lane, in rounds of the workgroup); then one sort per coordinate for the quantiles.
// The manifold and the mask are runtime values; every branch around a barrier is block-uniform.  No atomics, no scratch (scalars, as
// in nbp_ppe_kernel: an array indexed by a loop lives in scratch; the options are read through their pointer for the same reason).
__global__ void __launch_bounds__(512)
nbp_credible_kernel(NBP_CREDIBLE_ARGS) {
  extern __shared__ double smem[];
  const int P = nbp_credible_P(N);
  double *tab = smem, *X = smem + NBP_EXPTAB, *key = X + 3 * N;
  int32_t *idx = (int32_t *)(key + P);
  double *red = key + P + P / 2;
  const int b = blockIdx.x;
  const double *s = arena + S * slots[b];
  const int M = manifolds[b], K = masks[b], D = mani_dim(M), n = threadIdx.x;
  const int c = slot_count(s, N);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  nbp_exp_tab_init(tab);
  if (n < c)
    for (int k = 0; k < D; k++) X[k * N + n] = s[k * N + n];
  __syncthreads();
  const double mu0 = mean_geodesic_coord(X, c, M, 0, red);
  const double mu1 = D > 1 ? mean_geodesic_coord(X + N, c, M, 1, red) : 0.0;
  const double mu2 = D > 2 ? mean_geodesic_coord(X + 2 * N, c, M, 2, red) : 0.0;
  // ---- the own points --------------------------------------------------------------------------------------------------------
  const bool k0 = K & 1, k1 = D > 1 && (K & 2), k2 = D > 2 && (K & 4);
  const double h0 = k0 ? s[3 * N] : 1.0, h1 = k1 ? s[3 * N + 1] : 1.0, h2 = k2 ? s[3 * N + 2] : 1.0;
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1) & kde_bw_ok(h2);  // block-uniform
  const bool levels = valid && c >= 2;                               // (c == 1: there is no j != i)
  const bool c0 = is_circ(M, 0), c2 = is_circ(M, 2);
  double l = nan;
  if (levels && n < c) {
    const double x0 = k0 ? X[n] : 0.0, x1 = k1 ? X[N + n] : 0.0, x2 = k2 ? X[2 * N + n] : 0.0;
    l = cred_log_density(x0, x1, x2, X, N, c, n, k0, k1, k2, c0, c2, h0, h1, h2, tab);
  }
  if (logdens && n < N) logdens[(size_t)b * N + n] = l;
  // ---- the sort: positions c .. P - 1 hold +inf -------------------------------------------------------------------------------
  if (levels) {
    for (int p = n; p < P; p += blockDim.x) {  // (p >= blockDim.x lies beyond the count)
      key[p] = p < c ? l : INFINITY;
      idx[p] = p;
    }
    cred_sort(key, idx, P);
  }
  if (order)
    for (int p = n; p < N; p += blockDim.x) order[(size_t)b * N + p] = p < c ? (levels ? idx[p] : (valid ? p : -1)) : -1;
  // ---- the record: levels and counts ------------------------------------------------------------------------------------------
  nbp_credible_rec *r = rec + b;
  const int n_mass = opts->n_mass, n_prob = opts->n_prob;
  if (n < NBP_CRED_MAX) {
    double lev = 0.0;
    int inside = 0;
    if (n < n_mass) {
      lev = nan;
      if (levels) {
        int k = (int)ceil(opts->mass[n] * (double)c);
        k = k < 1 ? 1 : (k > c ? c : k);
        lev = key[c - k];
        inside = c - cred_first_at_or_above(key, c, lev, false);
      }
    }
    r->log_level[n] = lev;
    r->n_inside[n] = inside;
  }
  if (n == 0) {
    r->mean[0] = mu0;
    r->mean[1] = mu1;
    r->mean[2] = mu2;
    r->log_min = levels ? key[0] : nan;
    r->log_max = levels ? key[c - 1] : nan;
    r->count = c;
    r->pad = 0;
  }
  // ---- the queries of this belief ---------------------------------------------------------------------------------------------
  if (q_first) {
    const int q1 = q_first[b + 1];
    for (int q = q_first[b] + n; q < q1; q += blockDim.x) {
      const double *qq = queries + (size_t)NBP_MAXD * (size_t)q;
      double lq = nan, mass = nan;
      int above = -1;
      if (valid) {
        const double x0 = k0 ? qq[0] : 0.0, x1 = k1 ? qq[1] : 0.0, x2 = k2 ? qq[2] : 0.0;
        lq = cred_log_density(x0, x1, x2, X, N, c, -1, k0, k1, k2, c0, c2, h0, h1, h2, tab);
        if (levels) {
          above = c - cred_first_at_or_above(key, c, lq, true);
          mass = (double)above / (double)c;
        }
      }
      qrec[q].logdens = lq;
      qrec[q].mass = mass;
      qrec[q].n_above = above;
      qrec[q].pad = 0;
    }
  }
  // ---- the quantiles: one sort per coordinate of the manifold (the sorted l is no longer needed) -------------------------------
  for (int d = 0; d < NBP_MAXD; d++) {  // (block-uniform)
    double quant = 0.0;
    if (d < D) {
      const bool circ = is_circ(M, d);
      const double mu = d == 0 ? mu0 : (d == 1 ? mu1 : mu2);
      __syncthreads();  // the queries, or the lanes below, have read `key`
      for (int p = n; p < P; p += blockDim.x) {
        key[p] = p < c ? (circ ? stats_deviation(X[d * N + p], mu, true) : X[d * N + p]) : INFINITY;
        idx[p] = p;
      }
      cred_sort(key, idx, P);
      if (n < n_prob && n < NBP_CRED_MAX) {
        const double t = (double)(c - 1) * opts->prob[n];
        int lo = (int)floor(t);
        lo = lo < 0 ? 0 : (lo > c - 1 ? c - 1 : lo);  // (the host has checked the probability: this guards the LDS read alone)
        const int hi = lo + 1 < c - 1 ? lo + 1 : c - 1;
        const double vlo = key[lo], vhi = key[hi];
        quant = vlo + (t - (double)lo) * (vhi - vlo);
        if (circ) quant = wrap_pi(mu + quant);
      }
    }
    if (n < NBP_CRED_MAX) r->quant[d][n] = quant;
  }
}
#else
__global__ void nbp_credible_kernel(NBP_CREDIBLE_ARGS);
#endif

static inline size_t nbp_credible_lds_bytes(int N) {
  const size_t P = (size_t)nbp_credible_P(N);
  return ((size_t)NBP_EXPTAB + 3 * (size_t)N + P + P / 2 + NBP_RED) * 8;
}
