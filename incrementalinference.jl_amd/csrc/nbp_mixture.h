// nbp_mixture.h -- a resident belief summarised as a Gaussian mixture of K <= NBP_MIX_MAX components: weights, means and full
// covariances, fitted by hierarchical EM on the kernel centres of the belief's own KDE, all iterations in one launch.  DESIGN.md 3,
// "Mixture summaries", holds the definition; include/nbp.h states it at nbp_run_mixture.  Coordinates are tangent coordinates at the
// identity (Euclid(1-3); the circle; SE(2): x, y, theta in the world frame), c the count a slot holds, D the dimension, h the
// belief's bandwidth, delta(x, mu) = stats_deviation (wrapped on circular coordinates).
//   start     r_ik = 1 where particle i carries the label k, else 0 (label -1: in no component); mu_k = the given location; a
//             component is live when a particle below the count carries its label
//   M-step    n_k = sum_i r_ik; a live component with n_k < 0.5 is dropped for good; w_k = n_k / sum_{l live} n_l (l ascending);
//             mu_kd <- wrap(mu_kd + (sum_i r_ik delta_d(x_i, mu_k)) / n_k); then, delta about the NEW mean,
//             Sigma_kde = (sum_i (r_ik delta_d) delta_e) / n_k + [d = e] h_d h_d
//   E-step    Sigma_k = L L^T (closed form, rows in order); z = L^-1 delta by forward substitution with the reciprocals of the
//             diagonal; q = z_0 z_0 + z_1 z_1 + z_2 z_2; logdet = 2 (log L_00 + log L_11 + log L_22); tr = sum_d (h_d h_d) (Sigma^-1)_dd
//             from M = L^-1; cst_k = log w_k - 0.5 ((D log 2 pi + logdet) + tr); l_ik = cst_k - 0.5 q;
//             lse_i = m + log(sum_k exp(l_ik - m)), m = max_k l_ik, k ascending over the live components in one lane;
//             r_ik = exp(l_ik - lse_i) (exactly 0 below -700); J = (sum_i lse_i) / c
//   stop      after the E-step of iteration t >= 2 when tol > 0 and J_t - J_{t-1} <= tol (converged), or after max_iter iterations
//   result    live components ranked by weight descending, ties by the lower starting index; count_k = the particles whose greatest
//             r is r_ik (ties to the lower starting index); labels = the rank of that component
// A coordinate beyond D enters as delta = 0 with a unit diagonal: one written form for every manifold.  Sigma_k >= H in the Loewner
// order, so every pivot is >= h_d^2 > 0 up to rounding: no floor.  Every sum over the particles is reduced in one order: a butterfly
// inside each wave (wave_sum), the per-wave partials in LDS, one lane per sum adding them wave-ascending -- block_sum's additions.
// DEFINED here, unpinned.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"
#include "nbp_stats.h"  // stats_deviation

#define NBP_MIX_LOG_2PI 1.8378770664093453  // log(2 pi)
#define NBP_MIX_SUMS (NBP_MIX_MAX * 6)      // the most sums one reduction carries: six scatter entries per component
#define NBP_MIX_WAVES 8                     // waves of the largest workgroup (512 lanes)

#define NBP_MIXTURE_ARGS                                                                                               \
  const int32_t *slots, const int32_t *manifolds, const int32_t *labels_in, const double *init_mean, const double *arena, int N, \
      int64_t S, nbp_mixture_opts o, nbp_mixture_rec *recs, int32_t *labels_out
#if NBP_TU & NBP_TU_MIXTURE
// the reduction of up to NBP_MIX_SUMS sums at once.  mix_put: every lane of the workgroup hands in its term of sum s (wave-uniform s);
// mix_partials: after a barrier, the lane that owns sum s adds the partials wave-ascending.
__device__ __forceinline__ void mix_put(double v, double *part, int s) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[s * NBP_MIX_WAVES + (threadIdx.x >> 6)] = v;
}
__device__ __forceinline__ double mix_partials(const double *part, int s) {
  const int nw = (blockDim.x + 63) >> 6;
  double t = part[s * NBP_MIX_WAVES];
  for (int q = 1; q < nw; q++) t += part[s * NBP_MIX_WAVES + q];
  return t;
}

// the exponent of a responsibility: exp(a) for a <= 0, exactly 0 where exp_nonpos would clamp
__device__ __forceinline__ double mix_exp(double a, const double *tab) { return a < -700.0 ? 0.0 : exp_nonpos(a, tab); }

// l_ik of one particle under component k: par = (1 / L_00, 1 / L_11, 1 / L_22, L_10, L_20, L_21, cst), mu the component's mean
__device__ __forceinline__ double mix_loglik(double x0, double x1, double x2, const double *mu, const double *par, bool k1, bool k2,
                                             bool c0, bool c2) {
  const double d0 = stats_deviation(x0, mu[0], c0);
  const double d1 = k1 ? stats_deviation(x1, mu[1], false) : 0.0;
  const double d2 = k2 ? stats_deviation(x2, mu[2], c2) : 0.0;
  const double z0 = d0 * par[0];
  const double z1 = (d1 - par[3] * z0) * par[1];
  const double z2 = ((d2 - par[4] * z0) - par[5] * z1) * par[2];
  const double q = (z0 * z0 + z1 * z1) + z2 * z2;
  return par[6] - 0.5 * q;
}

// One workgroup per belief, 64 ceil(N / 64) lanes (the shape of nbp_meancov_kernel).  LDS: exp table | X[3][N] | part[48][8] |
// nk[8] | mu[8][3] | sig[8][6] | par[8][7] | jsum | cnt[8][8] (int32) | rnk[8] (int32).  Lane i owns point i and keeps its eight
// responsibilities in registers (the loops over k have a constant trip count and are unrolled: an array indexed by a runtime value
// lives in scratch); the set of live components is a block-uniform bit mask.  Per iteration: three reductions (the n_k; the mean
// sums; the scatter sums), the Cholesky factors formed by lanes 0 .. 7, the exponents, one reduction for J.  Every branch around a
// barrier is block-uniform.  The manifold is a runtime value.  No atomics, no scratch.
__global__ void __launch_bounds__(512)
nbp_mixture_kernel(NBP_MIXTURE_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *X = smem + NBP_EXPTAB, *part = X + 3 * N, *nk = part + NBP_MIX_SUMS * NBP_MIX_WAVES, *mu = nk + NBP_MIX_MAX;
  double *sig = mu + NBP_MIX_MAX * 3, *par = sig + NBP_MIX_MAX * 6, *jsum = par + NBP_MIX_MAX * 7;
  int32_t *cnt = (int32_t *)(jsum + 1), *rnk = cnt + NBP_MIX_MAX * NBP_MIX_WAVES;
  const int b = blockIdx.x, n = threadIdx.x, lane = n & 63, wv = n >> 6, nw = (blockDim.x + 63) >> 6;
  const double *s = arena + S * slots[b];
  const int M = manifolds[b], D = mani_dim(M);
  const int c = slot_count(s, N);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  nbp_exp_tab_init(tab);
  if (n < c)
    for (int k = 0; k < D; k++) X[k * N + n] = s[k * N + n];
  if (n < NBP_MIX_MAX * 3) mu[n] = init_mean[(size_t)b * NBP_MIX_MAX * NBP_MAXD + n];
  const bool k1 = D > 1, k2 = D > 2, c0 = is_circ(M, 0), c2 = is_circ(M, 2);
  const double h0 = s[3 * N], h1 = k1 ? s[3 * N + 1] : 1.0, h2 = k2 ? s[3 * N + 2] : 1.0;
  const bool mine = n < c;
  const int lab = (mine && n < N) ? labels_in[(size_t)b * N + n] : -1;
  // the live components: those whose label a particle below the count carries (a ballot per wave, the waves or-ed in order)
  {
    int m8 = 0;
#pragma unroll
    for (int k = 0; k < NBP_MIX_MAX; k++) m8 |= (__builtin_amdgcn_ballot_w64(lab == k) != 0ull) << k;
    if (lane == 0) cnt[wv] = m8;
  }
  __syncthreads();  // X, mu and the per-wave masks are written
  int live = 0;
  for (int q = 0; q < nw; q++) live |= cnt[q];
  __syncthreads();  // (`cnt` is written again behind the loop, which a belief without a fit does not enter)
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1) & kde_bw_ok(h2) & (live != 0);  // block-uniform
  const double x0 = mine ? X[n] : 0.0, x1 = (mine && k1) ? X[N + n] : 0.0, x2 = (mine && k2) ? X[2 * N + n] : 0.0;
  const double hh0 = h0 * h0, hh1 = k1 ? h1 * h1 : 0.0, hh2 = k2 ? h2 * h2 : 0.0;
  double r[NBP_MIX_MAX];
#pragma unroll
  for (int k = 0; k < NBP_MIX_MAX; k++) r[k] = lab == k ? 1.0 : 0.0;
  double J = nan, Jprev = nan;
  int it = 0, dropped = 0, conv = 0;
  while (valid && it < o.max_iter && !conv) {
    it++;
    // ---- M-step: the n_k ---------------------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < NBP_MIX_MAX; k++)
      if (live >> k & 1) mix_put(r[k], part, k);
    __syncthreads();
    if (n < NBP_MIX_MAX && (live >> n & 1)) nk[n] = mix_partials(part, n);
    __syncthreads();
    double tot = 0.0;
    for (int k = 0; k < NBP_MIX_MAX; k++)  // (every lane reads the same sums: the mask stays block-uniform)
      if (live >> k & 1) {
        if (nk[k] < 0.5) {
          live &= ~(1 << k);
          dropped++;
        } else {
          tot += nk[k];
        }
      }
    // ---- the means ---------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < NBP_MIX_MAX; k++)
      if (live >> k & 1) {
        mix_put(r[k] * stats_deviation(x0, mu[3 * k], c0), part, 3 * k);
        if (k1) mix_put(r[k] * stats_deviation(x1, mu[3 * k + 1], false), part, 3 * k + 1);
        if (k2) mix_put(r[k] * stats_deviation(x2, mu[3 * k + 2], c2), part, 3 * k + 2);
      }
    __syncthreads();
    if (n < NBP_MIX_MAX * 3 && (live >> (n / 3) & 1) && n % 3 < D) {
      const double v = mu[n] + mix_partials(part, n) / nk[n / 3];
      mu[n] = is_circ(M, n % 3) ? wrap_pi(v) : v;
    }
    __syncthreads();
    // ---- the covariances: scatter about the new mean, in the order 00 01 11 02 12 22 -----------------------------------------
#pragma unroll
    for (int k = 0; k < NBP_MIX_MAX; k++)
      if (live >> k & 1) {
        const double d0 = stats_deviation(x0, mu[3 * k], c0), rd0 = r[k] * d0;
        mix_put(rd0 * d0, part, 6 * k);
        if (k1) {
          const double d1 = stats_deviation(x1, mu[3 * k + 1], false), rd1 = r[k] * d1;
          mix_put(rd0 * d1, part, 6 * k + 1);
          mix_put(rd1 * d1, part, 6 * k + 2);
          if (k2) {
            const double d2 = stats_deviation(x2, mu[3 * k + 2], c2);
            mix_put(rd0 * d2, part, 6 * k + 3);
            mix_put(rd1 * d2, part, 6 * k + 4);
            mix_put((r[k] * d2) * d2, part, 6 * k + 5);
          }
        }
      }
    __syncthreads();
    if (n < NBP_MIX_MAX * 6 && (live >> (n / 6) & 1)) {
      const int e = n % 6;
      const bool used = e == 0 || (k1 && e <= 2) || k2;
      double v = e == 2 || e == 5 ? 1.0 : 0.0;  // beyond D: the unit matrix
      if (used) v = mix_partials(part, n) / nk[n / 6] + (e == 0 ? hh0 : (e == 2 ? hh1 : (e == 5 ? hh2 : 0.0)));
      sig[n] = v;
    }
    __syncthreads();
    // ---- E-step: the factors, by one lane per component ----------------------------------------------------------------------
    if (n < NBP_MIX_MAX && (live >> n & 1)) {
      const double *g = sig + 6 * n;
      const double l00 = sqrt(g[0]), i0 = 1.0 / l00;
      const double l10 = g[1] * i0, l11 = sqrt(g[2] - l10 * l10), i1 = 1.0 / l11;
      const double l20 = g[3] * i0, l21 = (g[4] - l20 * l10) * i1, l22 = sqrt((g[5] - l20 * l20) - l21 * l21), i2 = 1.0 / l22;
      const double m10 = -(l10 * i0) * i1, m21 = -(l21 * i1) * i2, m20 = -(l20 * i0 + l21 * m10) * i2;
      const double p00 = (i0 * i0 + m10 * m10) + m20 * m20, p11 = i1 * i1 + m21 * m21, p22 = i2 * i2;
      const double tr = (hh0 * p00 + hh1 * p11) + hh2 * p22;
      const double logdet = 2.0 * ((nbpm_log(l00) + nbpm_log(l11)) + nbpm_log(l22));
      double *p = par + 7 * n;
      p[0] = i0;
      p[1] = i1;
      p[2] = i2;
      p[3] = l10;
      p[4] = l20;
      p[5] = l21;
      p[6] = nbpm_log(nk[n] / tot) - 0.5 * (((double)D * NBP_MIX_LOG_2PI + logdet) + tr);
    }
    __syncthreads();
    // ---- the responsibilities --------------------------------------------------------------------------------------------------
    double lse = 0.0;
    {
      double l[NBP_MIX_MAX], mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NBP_MIX_MAX; k++) {
        l[k] = -INFINITY;
        if (live >> k & 1) {
          l[k] = mix_loglik(x0, x1, x2, mu + 3 * k, par + 7 * k, k1, k2, c0, c2);
          mx = fmax(mx, l[k]);
        }
      }
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NBP_MIX_MAX; k++)
        if (live >> k & 1) acc += mix_exp(l[k] - mx, tab);
      lse = mx + nbpm_log(acc);
#pragma unroll
      for (int k = 0; k < NBP_MIX_MAX; k++) r[k] = (mine && (live >> k & 1)) ? mix_exp(l[k] - lse, tab) : 0.0;
    }
    mix_put(mine ? lse : 0.0, part, 0);
    __syncthreads();
    if (n == 0) jsum[0] = mix_partials(part, 0);
    __syncthreads();
    Jprev = J;
    J = jsum[0] / (double)c;
    conv = (o.tol > 0.0 && it >= 2 && J - Jprev <= o.tol) ? 1 : 0;
  }
  // ---- the result ----------------------------------------------------------------------------------------------------------------
  // every particle's component: the greatest responsibility, ties to the lower index
  int best = -1;
  {
    double rb = -1.0;
#pragma unroll
    for (int k = 0; k < NBP_MIX_MAX; k++)
      if (valid && mine && (live >> k & 1) && r[k] > rb) {
        rb = r[k];
        best = k;
      }
  }
#pragma unroll
  for (int k = 0; k < NBP_MIX_MAX; k++) {
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(best == k);
    if (lane == 0) cnt[k * NBP_MIX_WAVES + wv] = __popcll(bal);
  }
  // the rank of a live component: by weight (n_k: the divisor is shared) descending, ties by the lower index
  if (n < NBP_MIX_MAX) {
    int rank = -1;
    if (valid && (live >> n & 1)) {
      rank = 0;
      for (int j = 0; j < NBP_MIX_MAX; j++)
        if ((live >> j & 1) && (nk[j] > nk[n] || (nk[j] == nk[n] && j < n))) rank++;
    }
    rnk[n] = rank;
  }
  __syncthreads();
  nbp_mixture_rec *rec = recs + b;
  const int n_comp = valid ? __popc(live) : 0;
  if (n < NBP_MIX_MAX) {  // lane n writes the record entries of RANK n
    int k = -1;
    for (int j = 0; j < NBP_MIX_MAX; j++)
      if (rnk[j] == n) k = j;
    const double fill = valid ? 0.0 : nan;
    double tot = 0.0;
    for (int j = 0; j < NBP_MIX_MAX; j++)
      if (valid && (live >> j & 1)) tot += nk[j];
    int members = 0;
    if (k >= 0)
      for (int q = 0; q < nw; q++) members += cnt[k * NBP_MIX_WAVES + q];
    rec->weight[n] = k >= 0 ? nk[k] / tot : fill;
    for (int d = 0; d < NBP_MAXD; d++) rec->mean[n][d] = (k >= 0 && d < D) ? mu[3 * k + d] : fill;
    const double *g = sig + 6 * (k >= 0 ? k : 0);
    const double g00 = k >= 0 ? g[0] : fill, g01 = (k >= 0 && k1) ? g[1] : fill, g11 = (k >= 0 && k1) ? g[2] : fill;
    const double g02 = (k >= 0 && k2) ? g[3] : fill, g12 = (k >= 0 && k2) ? g[4] : fill, g22 = (k >= 0 && k2) ? g[5] : fill;
    double *cv = rec->cov[n];
    cv[0] = g00;
    cv[1] = g01;
    cv[2] = g02;
    cv[3] = g01;
    cv[4] = g11;
    cv[5] = g12;
    cv[6] = g02;
    cv[7] = g12;
    cv[8] = g22;
    rec->count[n] = members;
  }
  if (n == 0) {
    rec->objective = J;
    rec->n_comp = n_comp;
    rec->iters = it;
    rec->converged = conv;
    rec->n_dropped = dropped;
  }
  if (labels_out && n < N) labels_out[(size_t)b * N + n] = best >= 0 ? rnk[best] : -1;
}
#else
__global__ void nbp_mixture_kernel(NBP_MIXTURE_ARGS);
#endif

static inline size_t nbp_mixture_lds_bytes(int N) {
  return ((size_t)NBP_EXPTAB + 3 * (size_t)N + NBP_MIX_SUMS * NBP_MIX_WAVES + NBP_MIX_MAX * (1 + 3 + 6 + 7) + 1) * 8 +
         (NBP_MIX_MAX * NBP_MIX_WAVES + NBP_MIX_MAX) * 4;
}
