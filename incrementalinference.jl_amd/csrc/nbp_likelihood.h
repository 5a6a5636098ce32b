// nbp_likelihood.h -- the likelihood of a factor's measurement model under the resident beliefs of its variables, any number of
// items (measurement model, slot A, slot B) in one launch.  DESIGN.md 3 ("Factor likelihoods") and include/nbp.h hold the definition:
//   zhat(a_i, b_j)  the root of the factor's residual (objective_t::normsq of nbp_device.h) in the measurement, tangent coordinates:
//                   LINREL b - a | CIRCULAR wrap_pi(b - a) | SE2 (c dx + s dy, -s dx + c dy, wrap_pi(b_th - a_th)), (s, c) =
//                   sincos(a_th) | EUCLIDDIST sqrt(sum_d (b_d - a_d)^2) | PRIOR a_i; a partial mask keeps its coordinates, ascending
//   log p_c(z)      Gaussian: delta = z - mean (wrapped on circular coordinates), L u = delta by forward substitution,
//                   -1/2 sum_k u_k^2 - (zd HALF_LOG_2PI + sum_k log L_kk); Uniform(a, a + w): -log w on [a, a + w], else -inf;
//                   Rayleigh(sigma): (log z - 2 log sigma) - z^2 / (2 sigma^2) for z > 0, else -inf
//   e_ijc           log(w_c / sum w) + log p_c(zhat_ij)
//   pass 1          M = max_ijc e_ijc
//   pass 2          S_c = sum_i sum_j exp(e_ijc - M), a term below exp(-700) dropped; j = 0 .. n_b - 1 in that order in the lane
//                   that owns i, the lanes added by block_sum
//   loglik          (M + log(sum_c S_c)) - log(n_a n_b);  comp_loglik[c] = (M + log S_c) - log(n_a n_b), -inf where S_c = 0
//   M = -inf        (nothing in the support): loglik and every comp_loglik[c], c < ncomp, are -inf
// One rounding per written operation.  Bandwidths are never read.
#pragma once
#include "nbp_kernels.h"


#define NBP_LIK_HALF_LOG_2PI 0.91893853320467274178  // log(2 pi) / 2

// one record per item
struct nbp_likelihood_rec {
  double loglik;
  double comp_loglik[NBP_MAXC];
};

#define NBP_LIKELIHOOD_ARGS const nbp_likelihood_desc *descs, const double *arena, int N, int64_t S, nbp_likelihood_rec *out
// the grouped kernel: the label rows of the two roles (-1: every point in group 0), table[n][8][8] and counts[n][2][8] out
#define NBP_MODE_LIKELIHOOD_ARGS                                                                                                 \
  const nbp_likelihood_desc *descs, const int32_t *row_a, const int32_t *row_b, const int32_t *labels, const double *arena, int N, \
      int64_t S, double *table, int32_t *counts
#if NBP_TU & (NBP_TU_LIKELIHOOD | NBP_TU_PRODUCTGRID)
// ---- shared with the local products on a grid (nbp_productgrid.h): the pair term and the component, the same bits there ----
// what a lane and a component bring to the pair loop: the lane's point (and the sine and cosine of its heading, formed once), the
// coordinates the mask keeps and whether each is circular (block-uniform), the component's parameters (block-uniform)
struct lik_lane {
  double a0, a1, a2, sn, cs;
  int D, s0, s1, s2;
  bool z0c, z1c, z2c;
};
struct lik_comp {
  double logw, lognorm;  // log(w_c / sum w); Gaussian: zd HALF_LOG_2PI + sum_k log L_kk, Uniform: log w, Rayleigh: 2 log sigma
  double m0, m1, m2, l00, l10, l11, l20, l21, l22;
};

__device__ __forceinline__ double lik_pick(double f0, double f1, double f2, int s) { return s == 0 ? f0 : (s == 1 ? f1 : f2); }

// e_ijc of one pair.  KIND, ZD (the measurement's dimension) and FAM are compile-time: the pair loops carry no branch on them.
template <int KIND, int ZD, int FAM>
__device__ __forceinline__ double lik_term(const lik_lane &l, const lik_comp &k, double b0, double b1, double b2) {
  double f0, f1 = 0.0, f2 = 0.0;
  if (KIND == NBP_F_PRIOR) {
    f0 = l.a0;
    f1 = l.a1;
    f2 = l.a2;
  } else if (KIND == NBP_F_LINREL) {
    f0 = b0 - l.a0;
    f1 = b1 - l.a1;
    f2 = b2 - l.a2;
  } else if (KIND == NBP_F_CIRCULAR) {
    f0 = wrap_pi(b0 - l.a0);
  } else if (KIND == NBP_F_SE2) {
    const double dx = b0 - l.a0, dy = b1 - l.a1;
    f0 = l.cs * dx + l.sn * dy;
    f1 = -l.sn * dx + l.cs * dy;
    f2 = wrap_pi(b2 - l.a2);
  } else {  // NBP_F_EUCLIDDIST
    double q = (b0 - l.a0) * (b0 - l.a0);
    if (l.D > 1) q += (b1 - l.a1) * (b1 - l.a1);
    if (l.D > 2) q += (b2 - l.a2) * (b2 - l.a2);
    f0 = sqrt(q);
  }
  const double z0 = lik_pick(f0, f1, f2, l.s0);
  double lp;
  if (FAM == NBP_DIST_GAUSSIAN) {
    double d0 = z0 - k.m0;
    if (l.z0c) d0 = wrap_pi(d0);
    const double u0 = d0 / k.l00;
    double q = u0 * u0;
    if (ZD > 1) {
      double d1 = lik_pick(f0, f1, f2, l.s1) - k.m1;
      if (l.z1c) d1 = wrap_pi(d1);
      const double u1 = (d1 - k.l10 * u0) / k.l11;
      q += u1 * u1;
      if (ZD > 2) {
        double d2 = lik_pick(f0, f1, f2, l.s2) - k.m2;
        if (l.z2c) d2 = wrap_pi(d2);
        const double u2 = ((d2 - k.l20 * u0) - k.l21 * u1) / k.l22;
        q += u2 * u2;
      }
    }
    lp = -0.5 * q - k.lognorm;
  } else if (FAM == NBP_DIST_UNIFORM) {
    lp = (z0 >= k.m0 && z0 <= k.m0 + k.l00) ? -k.lognorm : -INFINITY;
  } else {  // NBP_DIST_RAYLEIGH
    // (nbpm_log takes positive normal numbers: the select keeps it off the others, whose lanes get -inf)
    const bool in = z0 > 0.0;
    const double v = (nbpm_log(in ? z0 : 1.0) - k.lognorm) - (z0 * z0) / (2.0 * (k.l00 * k.l00));
    lp = in ? v : -INFINITY;
  }
  return k.logw + lp;
}

#endif
#if NBP_TU & NBP_TU_LIKELIHOOD
// one pass of lane i over j = 0 .. cb - 1 for one component: PASS 0 the maximum of e, PASS 1 the sum of exp(e - M).  B in LDS, every
// lane of a wave reads the same address (broadcast).  A unary item has cb = 1 and reads no B.
template <int KIND, int ZD, int FAM, int PASS>
__device__ __forceinline__ double lik_scan(const lik_lane &l, const lik_comp &k, const double *B, int N, int cb, double M, const double *tab) {
  double acc = PASS ? 0.0 : -INFINITY;
  for (int j = 0; j < cb; j++) {
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (KIND != NBP_F_PRIOR) {
      b0 = B[j];
      if (l.D > 1) b1 = B[N + j];
      if (l.D > 2) b2 = B[2 * N + j];
    }
    const double e = lik_term<KIND, ZD, FAM>(l, k, b0, b1, b2);
    if (PASS) {
      const double d = e - M;
      acc += d >= -700.0 ? exp_nonpos(d, tab) : 0.0;  // (-inf and NaN fail the comparison as well)
    } else
      acc = fmax(acc, e);
  }
  return acc;
}

// kind, measurement dimension and family are block-uniform runtime values: one dispatch per component and pass, outside the pair loop
template <int KIND, int ZD, int PASS>
__device__ __forceinline__ double lik_scan_fam(int fam, const lik_lane &l, const lik_comp &k, const double *B, int N, int cb, double M,
                                               const double *tab) {
  if (ZD == 1 && fam == NBP_DIST_UNIFORM) return lik_scan<KIND, ZD, NBP_DIST_UNIFORM, PASS>(l, k, B, N, cb, M, tab);
  if (ZD == 1 && fam == NBP_DIST_RAYLEIGH) return lik_scan<KIND, ZD, NBP_DIST_RAYLEIGH, PASS>(l, k, B, N, cb, M, tab);
  return lik_scan<KIND, ZD, NBP_DIST_GAUSSIAN, PASS>(l, k, B, N, cb, M, tab);
}
template <int KIND, int PASS>
__device__ __forceinline__ double lik_scan_zd(int zd, int fam, const lik_lane &l, const lik_comp &k, const double *B, int N, int cb,
                                              double M, const double *tab) {
  if (KIND == NBP_F_CIRCULAR || KIND == NBP_F_EUCLIDDIST || zd == 1) return lik_scan_fam<KIND, 1, PASS>(fam, l, k, B, N, cb, M, tab);
  if (zd == 2) return lik_scan_fam<KIND, 2, PASS>(fam, l, k, B, N, cb, M, tab);
  return lik_scan_fam<KIND, 3, PASS>(fam, l, k, B, N, cb, M, tab);
}
template <int PASS>
__device__ __forceinline__ double lik_scan_kind(int kind, int zd, int fam, const lik_lane &l, const lik_comp &k, const double *B, int N,
                                                int cb, double M, const double *tab) {
  switch (kind) {
    case NBP_F_PRIOR: return lik_scan_zd<NBP_F_PRIOR, PASS>(zd, fam, l, k, B, N, cb, M, tab);
    case NBP_F_LINREL: return lik_scan_zd<NBP_F_LINREL, PASS>(zd, fam, l, k, B, N, cb, M, tab);
    case NBP_F_CIRCULAR: return lik_scan_zd<NBP_F_CIRCULAR, PASS>(zd, fam, l, k, B, N, cb, M, tab);
    case NBP_F_SE2: return lik_scan_zd<NBP_F_SE2, PASS>(zd, fam, l, k, B, N, cb, M, tab);
    default: return lik_scan_zd<NBP_F_EUCLIDDIST, PASS>(zd, fam, l, k, B, N, cb, M, tab);
  }
}

#endif
#if NBP_TU & (NBP_TU_LIKELIHOOD | NBP_TU_PRODUCTGRID)
// component c of the descriptor as the pair loops read it (block-uniform: every lane forms the same values)
__device__ __forceinline__ lik_comp lik_component(const nbp_likelihood_desc *d, int c, int zd, int fam, double wsum) {
  const double *p = d->comp[c];
  lik_comp k;
  k.logw = p[0] > 0.0 ? nbpm_log(p[0] / wsum) : -INFINITY;
  k.m0 = p[1];
  k.m1 = p[2];
  k.m2 = p[3];
  k.l00 = p[4];
  k.l10 = p[7];
  k.l11 = p[8];
  k.l20 = p[10];
  k.l21 = p[11];
  k.l22 = p[12];
  if (fam == NBP_DIST_UNIFORM) k.lognorm = nbpm_log(k.l00);
  else if (fam == NBP_DIST_RAYLEIGH) k.lognorm = 2.0 * nbpm_log(k.l00);
  else {
    double s = nbpm_log(k.l00);
    if (zd > 1) s += nbpm_log(k.l11);
    if (zd > 2) s += nbpm_log(k.l22);
    k.lognorm = (double)zd * NBP_LIK_HALF_LOG_2PI + s;
  }
  return k;
}

#endif
#if NBP_TU & NBP_TU_LIKELIHOOD
// One workgroup per item, 64 ceil(N / 64) lanes (at most 512).  LDS: exp table | B[3][N] | red | S_c[NBP_MAXC].  Lane i owns a_i;
// per component two passes over j, the maximum over the whole item between them (block_max), the lanes' sums added by block_sum;
// lane 0 writes the record.  A value depends on the item alone.  No atomics.  The host has checked the descriptor.
__global__ void __launch_bounds__(512)
nbp_likelihood_kernel(NBP_LIKELIHOOD_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *B = smem + NBP_EXPTAB, *red = B + 3 * N, *Sc = red + NBP_RED;
  const nbp_likelihood_desc *d = descs + blockIdx.x;
  const int kind = d->kind, M = d->manifold, D = mani_dim(M), n = threadIdx.x, ncomp = d->ncomp;
  const bool unary = kind == NBP_F_PRIOR;
  const double *sa = arena + S * d->slot_a, *sb = unary ? sa : arena + S * d->slot_b;
  const int ca = slot_count(sa, N), cb = unary ? 1 : slot_count(sb, N);
  nbp_exp_tab_init(tab);
  if (!unary && n < cb)
    for (int k = 0; k < D; k++) B[k * N + n] = sb[k * N + n];
  __syncthreads();
  // the coordinates of the measurement: those of the mask in ascending order (no mask: all the kind has)
  const int full = (kind == NBP_F_CIRCULAR || kind == NBP_F_EUCLIDDIST) ? 1 : (1 << D) - 1;
  const int mask = d->partial_mask ? d->partial_mask : full;
  const int zd = __popc(mask);
  lik_lane l;
  l.D = D;
  l.s0 = __ffs(mask) - 1;
  const int rest = mask & (mask - 1);
  l.s1 = rest ? __ffs(rest) - 1 : 0;
  l.s2 = 2;
  // circular: the angle of CircularCircular, the heading of an SE(2) factor, a prior's coordinates as its manifold has them
  const bool cf0 = kind == NBP_F_CIRCULAR || (unary && is_circ(M, 0)), cf2 = kind == NBP_F_SE2 || (unary && is_circ(M, 2));
  l.z0c = l.s0 == 0 ? cf0 : (l.s0 == 2 && cf2);
  l.z1c = l.s1 == 2 && cf2;
  l.z2c = cf2;
  const bool mine = n < ca;
  l.a0 = mine ? sa[n] : 0.0;
  l.a1 = (mine && D > 1) ? sa[N + n] : 0.0;
  l.a2 = (mine && D > 2) ? sa[2 * N + n] : 0.0;
  l.sn = 0.0;
  l.cs = 1.0;
  if (kind == NBP_F_SE2) sincos_fast(l.a2, &l.sn, &l.cs);
  double wsum = 0.0;
  for (int c = 0; c < ncomp; c++) wsum += d->comp[c][0];

  // ---- pass 1: the maximum over every pair and component ----
  double mx = -INFINITY;
  for (int c = 0; c < ncomp; c++) {
    const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
    const lik_comp k = lik_component(d, c, zd, fam, wsum);
    const double m = lik_scan_kind<0>(kind, zd, fam, l, k, B, N, cb, 0.0, tab);
    if (mine) mx = fmax(mx, m);
  }
  const double Mx = block_max(mx, red);

  // ---- pass 2: the sums relative to it, one per component ----
  if (Mx > -INFINITY) {  // (block-uniform)
    for (int c = 0; c < ncomp; c++) {
      const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
      const lik_comp k = lik_component(d, c, zd, fam, wsum);
      const double s = lik_scan_kind<1>(kind, zd, fam, l, k, B, N, cb, Mx, tab);
      const double t = block_sum(mine ? s : 0.0, red);
      if (n == 0) Sc[c] = t;
    }
  }
  if (n == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    nbp_likelihood_rec *r = out + blockIdx.x;
    const double ln = nbpm_log((double)ca * (double)cb);
    double tot = 0.0;
    for (int c = 0; c < NBP_MAXC; c++) {
      double v = nan;
      if (c < ncomp) {
        const double s = Mx > -INFINITY ? Sc[c] : 0.0;
        tot += s;
        v = s > 0.0 ? (Mx + nbpm_log(s)) - ln : -INFINITY;
      }
      r->comp_loglik[c] = v;
    }
    r->loglik = tot > 0.0 ? (Mx + nbpm_log(tot)) - ln : -INFINITY;
  }
}

// ---- the same likelihood, group by group ("Joint hypotheses"; include/nbp.h, nbp_run_factor_mode_likelihood) ---------
// Every particle of A and of B carries a label in -1 .. NBP_MAXK - 1 (the rank of its mode); cell (k, l) of the item's table is
// the likelihood over the pairs with a_i in group k and b_j in group l:
//   pass 1   M_kl = max over i in k, j in l, c of e_ijc
//   pass 2   S_klc = sum_{i in k} sum_{j in l} exp(e_ijc - M_kl): j ascending in the lane that owns i, the lanes added by block_sum
//            with an exact zero in every lane outside k, the components added in ascending c
//   T[k, l]  (M_kl + log sum_c S_klc) - log(n_k n_l); -inf where M_kl = -inf; NaN where n_k = 0 or n_l = 0
// One workgroup per item, 64 ceil(N / 64) lanes.  LDS: exp table | B[3][N] | red | M[8][8] | S[8][8] | wave counts[8][16] |
// counts[16].  B is staged SORTED BY GROUP, stably (a point's place: the points of lower groups, the points of its group in the
// waves before, the points of its group in the lanes before: ballots, no atomics), and the points labelled -1 are not staged.  So
// column l is one contiguous run of B in ascending j, and lik_scan walks it exactly as the ungrouped kernel walks the whole of B:
// a lane keeps ONE accumulator per pass, nothing is indexed at run time and nothing is selected inside the pair loop.  Skipping
// the pairs of other groups and adding an exact zero for them are the same number, so with one group on either side the cell is
// nbp_likelihood_kernel's loglik bit for bit.  The reductions run per PRESENT cell (the counts are block-uniform): a unimodal
// pair makes one block_max and ncomp block_sums, as the ungrouped kernel does.  Row -1: every point within the count in group 0.
__global__ void __launch_bounds__(512)
nbp_mode_likelihood_kernel(NBP_MODE_LIKELIHOOD_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *B = smem + NBP_EXPTAB, *red = B + 3 * N, *Mt = red + NBP_RED, *St = Mt + NBP_MAXK * NBP_MAXK;
  int *cntw = (int *)(St + NBP_MAXK * NBP_MAXK), *cnt = cntw + 8 * 2 * NBP_MAXK;
  const nbp_likelihood_desc *d = descs + blockIdx.x;
  const int kind = d->kind, M = d->manifold, D = mani_dim(M), n = threadIdx.x, ncomp = d->ncomp;
  const int lane = n & 63, w = n >> 6, nw = (blockDim.x + 63) >> 6;
  const bool unary = kind == NBP_F_PRIOR;
  const double *sa = arena + S * d->slot_a, *sb = unary ? sa : arena + S * d->slot_b;
  const int ca = slot_count(sa, N), cb = unary ? 1 : slot_count(sb, N);
  const int ra = row_a[blockIdx.x], rb = unary ? -1 : row_b[blockIdx.x];
  nbp_exp_tab_init(tab);
  // the groups of this lane's a_i and b_j (the host has checked the range; anything else counts as -1 here as well)
  int la = -1, lb = -1;
  if (n < ca) la = ra < 0 ? 0 : labels[(size_t)ra * N + n];
  if (n < cb) lb = rb < 0 ? 0 : labels[(size_t)rb * N + n];
  if ((unsigned)la >= NBP_MAXK) la = -1;
  if ((unsigned)lb >= NBP_MAXK) lb = -1;
  if (n < NBP_MAXK * NBP_MAXK) St[n] = 0.0;
  // members per wave, and this lane's rank among the lanes of its wave in the same group of B
  const unsigned long long below = (1ull << lane) - 1ull;
  int rank = 0;
  for (int g = 0; g < NBP_MAXK; g++) {
    const unsigned long long ma = __ballot(la == g), mb = __ballot(lb == g);
    if (lane == 0) {
      cntw[w * 2 * NBP_MAXK + g] = __popcll(ma);
      cntw[w * 2 * NBP_MAXK + NBP_MAXK + g] = __popcll(mb);
    }
    if (lb == g) rank = __popcll(mb & below);
  }
  __syncthreads();
  if (n < 2 * NBP_MAXK) {
    int t = 0;
    for (int i = 0; i < nw; i++) t += cntw[i * 2 * NBP_MAXK + n];
    cnt[n] = t;
    counts[(size_t)blockIdx.x * 2 * NBP_MAXK + n] = t;
  }
  __syncthreads();
  if (!unary && lb >= 0) {
    int pos = rank;
    for (int g = 0; g < lb; g++) pos += cnt[NBP_MAXK + g];
    for (int i = 0; i < w; i++) pos += cntw[i * 2 * NBP_MAXK + NBP_MAXK + lb];
    for (int k = 0; k < D; k++) B[k * N + pos] = sb[k * N + n];  // (pos < the members of B <= cb <= N)
  }
  __syncthreads();
  // the coordinates of the measurement, the lane's point: as nbp_likelihood_kernel forms them
  const int full = (kind == NBP_F_CIRCULAR || kind == NBP_F_EUCLIDDIST) ? 1 : (1 << D) - 1;
  const int mask = d->partial_mask ? d->partial_mask : full;
  const int zd = __popc(mask);
  lik_lane l;
  l.D = D;
  l.s0 = __ffs(mask) - 1;
  const int rest = mask & (mask - 1);
  l.s1 = rest ? __ffs(rest) - 1 : 0;
  l.s2 = 2;
  const bool cf0 = kind == NBP_F_CIRCULAR || (unary && is_circ(M, 0)), cf2 = kind == NBP_F_SE2 || (unary && is_circ(M, 2));
  l.z0c = l.s0 == 0 ? cf0 : (l.s0 == 2 && cf2);
  l.z1c = l.s1 == 2 && cf2;
  l.z2c = cf2;
  const bool mine = n < ca;
  l.a0 = mine ? sa[n] : 0.0;
  l.a1 = (mine && D > 1) ? sa[N + n] : 0.0;
  l.a2 = (mine && D > 2) ? sa[2 * N + n] : 0.0;
  l.sn = 0.0;
  l.cs = 1.0;
  if (kind == NBP_F_SE2) sincos_fast(l.a2, &l.sn, &l.cs);
  double wsum = 0.0;
  for (int c = 0; c < ncomp; c++) wsum += d->comp[c][0];

  // ---- pass 1: the maximum of every present cell ----
  int at = 0;
  for (int g = 0; g < NBP_MAXK; g++) {  // (column g of the table: B[at .. at + ng))
    const int ng = cnt[NBP_MAXK + g];
    if (ng == 0) continue;  // (block-uniform)
    double mx = -INFINITY;
    for (int c = 0; c < ncomp; c++) {
      const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
      const lik_comp k = lik_component(d, c, zd, fam, wsum);
      mx = fmax(mx, lik_scan_kind<0>(kind, zd, fam, l, k, B + at, N, ng, 0.0, tab));
    }
    for (int r = 0; r < NBP_MAXK; r++) {
      if (cnt[r] == 0) continue;
      const double m = block_max(la == r ? mx : -INFINITY, red);
      if (n == 0) Mt[r * NBP_MAXK + g] = m;
    }
    at += ng;
  }
  __syncthreads();

  // ---- pass 2: the sums of every present cell relative to its own maximum, the components added in ascending c ----
  at = 0;
  for (int g = 0; g < NBP_MAXK; g++) {
    const int ng = cnt[NBP_MAXK + g];
    if (ng == 0) continue;
    const double Mx = la >= 0 ? Mt[la * NBP_MAXK + g] : INFINITY;  // (a lane outside every group adds zeros, and they are masked)
    for (int c = 0; c < ncomp; c++) {
      const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
      const lik_comp k = lik_component(d, c, zd, fam, wsum);
      const double s = lik_scan_kind<1>(kind, zd, fam, l, k, B + at, N, ng, Mx, tab);
      for (int r = 0; r < NBP_MAXK; r++) {
        if (cnt[r] == 0) continue;
        const double t = block_sum(la == r ? s : 0.0, red);
        if (n == 0) St[r * NBP_MAXK + g] += t;
      }
    }
    at += ng;
  }
  __syncthreads();
  if (n < NBP_MAXK * NBP_MAXK) {
    const int r = n / NBP_MAXK, g = n % NBP_MAXK, nr = cnt[r], ng = cnt[NBP_MAXK + g];
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (nr > 0 && ng > 0) {
      const double Mx = Mt[n], tot = Mx > -INFINITY ? St[n] : 0.0;
      v = tot > 0.0 ? (Mx + nbpm_log(tot)) - nbpm_log((double)nr * (double)ng) : -INFINITY;
    }
    table[(size_t)blockIdx.x * NBP_MAXK * NBP_MAXK + n] = v;
  }
}
#else
__global__ void nbp_likelihood_kernel(NBP_LIKELIHOOD_ARGS);
__global__ void nbp_mode_likelihood_kernel(NBP_MODE_LIKELIHOOD_ARGS);
#endif

static inline size_t nbp_likelihood_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 3 * (size_t)N + NBP_RED + NBP_MAXC) * 8; }
static inline size_t nbp_mode_likelihood_lds_bytes(int N) {
  return ((size_t)NBP_EXPTAB + 3 * (size_t)N + NBP_RED + 2 * NBP_MAXK * NBP_MAXK) * 8 + ((size_t)8 * 2 * NBP_MAXK + 2 * NBP_MAXK) * 4;
}
