// nbp_overlap.h -- how much two resident beliefs overlap, for listed pairs and as a search over a list of beliefs.  DESIGN.md 3
// ("Belief overlaps") and include/nbp.h hold the definition.  Belief a: n points, bandwidth h_a, coordinate mask K_a on its
// manifold; belief b: m points, h_b, K_b.  The masked coordinates are taken in ascending order: position k of a goes with
// position k of b (the host has checked that they agree in number, D_K, and in kind).
//   s_k     h_a,k h_a,k + h_b,k h_b,k;  r_k = 1 / s_k
//   e_ij    -1/2 (delta_0^2 r_0 + delta_1^2 r_1 + delta_2^2 r_2) over the D_K positions, in that order; delta_k = a_i,k - b_j,k,
//           wrapped to [-pi, pi) on circular positions
//   pass 1  M = max_ij e_ij
//   pass 2  S = sum_i sum_j exp(e_ij - M), a term below exp(-700) dropped; j = 0 .. m - 1 in that order in the lane that owns i,
//           the lanes added by block_sum
//   L_ab    ((M + log S) - log(n m)) - sum_k 1/2 log(2 pi s_k), the sum over k in position order
//   logc    L_ab - 1/2 (L_aa + L_bb); the three L from ov_cross, the ONE function and the one order: a belief against a
//           bit-identical copy, or against its own slot, gives exactly 0.0
// A bandwidth entry IN the mask of either belief that is not positive and finite (or an s_k that is not): every value is NaN.
// One rounding per written operation.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"


// what nbp_overlap_prep_kernel leaves per listed belief for the search: the box of its points on every masked position, the
// masked bandwidth, L_aa, and whether the bandwidth is usable
struct nbp_overlap_prep {
  double lo[NBP_MAXD], hi[NBP_MAXD], h[NBP_MAXD];
  double laa;
  int32_t valid, count;
};

#define NBP_OVERLAP_ARGS                                                                                                        \
  const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds_a, const int32_t *manifolds_b, const int32_t *masks_a, \
      const int32_t *masks_b, const double *arena, int N, int64_t S, nbp_overlap_rec *out
#define NBP_OVERLAP_PREP_ARGS \
  const int32_t *slots, const int32_t *manifolds, const int32_t *masks, const double *arena, int N, int64_t S, nbp_overlap_prep *prep
// reach2 = reach * reach and logmin = log(min_coeff), both formed on the host
#define NBP_OVERLAP_SEARCH_ARGS                                                                                                 \
  const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int V, const double *arena, int N, int64_t S,            \
      const nbp_overlap_prep *prep, double reach2, double logmin, int topk, int32_t *idx_out, double *logc_out, int32_t *found_out, \
      int32_t *evaluated_out
#if NBP_TU & NBP_TU_OVERLAP
// the masked coordinates of a belief in ascending order, and whether each is circular (block-uniform)
struct ov_geom {
  int DK, k0, k1, k2;
  bool c0, c1, c2;
};
__device__ __forceinline__ ov_geom ov_geometry(int M, int mask) {
  ov_geom g;
  g.DK = __popc(mask);
  g.k0 = __ffs(mask) - 1;
  const int rest = mask & (mask - 1);
  g.k1 = rest ? __ffs(rest) - 1 : 0;
  g.k2 = 2;
  g.c0 = is_circ(M, g.k0);
  g.c1 = g.DK > 1 && is_circ(M, g.k1);
  g.c2 = g.DK > 2 && is_circ(M, g.k2);
  return g;
}
// the masked coordinate rows of a slot into LDS, position k in X[k N ..]; lane i brings point i
__device__ __forceinline__ void ov_stage(double *X, const double *s, int N, int cnt, const ov_geom &g) {
  const int n = threadIdx.x;
  if (n < cnt) {
    X[n] = s[g.k0 * N + n];
    if (g.DK > 1) X[N + n] = s[g.k1 * N + n];
    if (g.DK > 2) X[2 * N + n] = s[g.k2 * N + n];
  }
}
// the masked bandwidth of a slot; positions beyond D_K carry 1
__device__ __forceinline__ void ov_bandwidth(const double *s, int N, const ov_geom &g, double *h0, double *h1, double *h2) {
  *h0 = s[3 * N + g.k0];
  *h1 = g.DK > 1 ? s[3 * N + g.k1] : 1.0;
  *h2 = g.DK > 2 ? s[3 * N + g.k2] : 1.0;
}

// what a pair of bandwidths brings to the pair loop (block-uniform)
struct ov_pair {
  double r0, r1, r2, norm;
  bool ok;
};
__device__ __forceinline__ ov_pair ov_setup(int DK, double ha0, double ha1, double ha2, double hb0, double hb1, double hb2) {
  const double s0 = ha0 * ha0 + hb0 * hb0, s1 = DK > 1 ? ha1 * ha1 + hb1 * hb1 : 1.0, s2 = DK > 2 ? ha2 * ha2 + hb2 * hb2 : 1.0;
  ov_pair p;
  p.ok = kde_bw_ok(ha0) & kde_bw_ok(ha1) & kde_bw_ok(ha2) & kde_bw_ok(hb0) & kde_bw_ok(hb1) & kde_bw_ok(hb2) & kde_bw_ok(s0) &
         kde_bw_ok(s1) & kde_bw_ok(s2);
  p.r0 = 1.0 / s0;
  p.r1 = 1.0 / s1;
  p.r2 = 1.0 / s2;
  // (nbpm_log takes positive normal numbers: the select keeps it off the others, whose records are NaN)
  double nm = 0.5 * nbpm_log(NBP_TWO_PI * (p.ok ? s0 : 1.0));
  if (DK > 1) nm += 0.5 * nbpm_log(NBP_TWO_PI * (p.ok ? s1 : 1.0));
  if (DK > 2) nm += 0.5 * nbpm_log(NBP_TWO_PI * (p.ok ? s2 : 1.0));
  p.norm = nm;
  return p;
}

// one pass of the lane that owns x over j = 0 .. m - 1: PASS 0 the maximum of e, PASS 1 the sum of exp(e - M).  Y in LDS, every
// lane of a wave reads the same address (broadcast).  DK and whether any position wraps are compile-time.
template <int DK, bool CIRC, int PASS>
__device__ __forceinline__ double ov_scan(double x0, double x1, double x2, const double *Y, int N, int m, const ov_geom &g, const ov_pair &p,
                                          double M, const double *tab) {
  double acc = PASS ? 0.0 : -INFINITY;
  for (int j = 0; j < m; j++) {
    double d0 = x0 - Y[j];
    if (CIRC && g.c0) d0 = wrap_pi(d0);
    double q = (d0 * d0) * p.r0;
    if (DK > 1) {
      double d1 = x1 - Y[N + j];
      if (CIRC && g.c1) d1 = wrap_pi(d1);
      q += (d1 * d1) * p.r1;
    }
    if (DK > 2) {
      double d2 = x2 - Y[2 * N + j];
      if (CIRC && g.c2) d2 = wrap_pi(d2);
      q += (d2 * d2) * p.r2;
    }
    const double e = -0.5 * q;
    if (PASS) {
      const double d = e - M;
      acc += d >= -700.0 ? exp_nonpos(d, tab) : 0.0;
    } else
      acc = fmax(acc, e);
  }
  return acc;
}
template <int PASS>
__device__ __forceinline__ double ov_scan_dk(double x0, double x1, double x2, const double *Y, int N, int m, const ov_geom &g,
                                             const ov_pair &p, double M, const double *tab) {
  const bool circ = g.c0 | g.c1 | g.c2;  // block-uniform, like DK: one dispatch per pass, outside the pair loop
  if (g.DK == 1) return circ ? ov_scan<1, true, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab) : ov_scan<1, false, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab);
  if (g.DK == 2) return circ ? ov_scan<2, true, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab) : ov_scan<2, false, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab);
  return circ ? ov_scan<3, true, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab) : ov_scan<3, false, PASS>(x0, x1, x2, Y, N, m, g, p, M, tab);
}

// L_xy: the one function, and the one order, behind L_aa, L_bb and L_ab in every kernel of this file.  X (nx points, the lanes own
// them) and Y (ny points, walked) in LDS, nx, ny >= 1, p.ok.  Every lane of the workgroup calls and receives the value.
__device__ __forceinline__ double ov_cross(const double *X, int nx, const double *Y, int ny, int N, const ov_geom &g, const ov_pair &p,
                                           double *red, const double *tab) {
  const int n = threadIdx.x;
  const bool mine = n < nx;
  const double x0 = mine ? X[n] : 0.0, x1 = (mine && g.DK > 1) ? X[N + n] : 0.0, x2 = (mine && g.DK > 2) ? X[2 * N + n] : 0.0;
  double mx = -INFINITY;
  if (mine) mx = ov_scan_dk<0>(x0, x1, x2, Y, N, ny, g, p, 0.0, tab);
  const double Mx = block_max(mx, red);
  double s = 0.0;
  if (mine) s = ov_scan_dk<1>(x0, x1, x2, Y, N, ny, g, p, Mx, tab);
  const double sum = block_sum(s, red);  // >= 1: the pair of the maximum adds exp(0)
  return ((Mx + nbpm_log(sum)) - nbpm_log((double)nx * (double)ny)) - p.norm;
}

// One workgroup per pair, 64 ceil(N / 64) lanes (at most 512).  LDS: exp table | A[3][N] | B[3][N] | red.  The two passes three
// times (aa, bb, ab) through ov_cross; lane 0 writes the record.  A value depends on the pair alone.  No atomics.
__global__ void __launch_bounds__(512)
nbp_overlap_kernel(NBP_OVERLAP_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *A = smem + NBP_EXPTAB, *B = A + 3 * N, *red = B + 3 * N;
  const double *sa = arena + S * slots_a[blockIdx.x], *sb = arena + S * slots_b[blockIdx.x];
  const ov_geom ga = ov_geometry(manifolds_a[blockIdx.x], masks_a[blockIdx.x]), gb = ov_geometry(manifolds_b[blockIdx.x], masks_b[blockIdx.x]);
  const int ca = slot_count(sa, N), cb = slot_count(sb, N);
  nbp_exp_tab_init(tab);
  ov_stage(A, sa, N, ca, ga);
  ov_stage(B, sb, N, cb, gb);
  __syncthreads();
  double ha0, ha1, ha2, hb0, hb1, hb2;
  ov_bandwidth(sa, N, ga, &ha0, &ha1, &ha2);
  ov_bandwidth(sb, N, gb, &hb0, &hb1, &hb2);
  const ov_pair paa = ov_setup(ga.DK, ha0, ha1, ha2, ha0, ha1, ha2), pbb = ov_setup(ga.DK, hb0, hb1, hb2, hb0, hb1, hb2),
                pab = ov_setup(ga.DK, ha0, ha1, ha2, hb0, hb1, hb2);
  const bool valid = paa.ok & pbb.ok & pab.ok;  // block-uniform
  double laa = 0.0, lbb = 0.0, lab = 0.0;
  if (valid) {
    laa = ov_cross(A, ca, A, ca, N, ga, paa, red, tab);
    lbb = ov_cross(B, cb, B, cb, N, ga, pbb, red, tab);
    lab = ov_cross(A, ca, B, cb, N, ga, pab, red, tab);
  }
  if (threadIdx.x == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    nbp_overlap_rec *r = out + blockIdx.x;
    r->logc = valid ? lab - 0.5 * (laa + lbb) : nan;
    r->lab = valid ? lab : nan;
    r->laa = valid ? laa : nan;
    r->lbb = valid ? lbb : nan;
  }
}

// One workgroup per listed belief, the same lanes.  LDS: exp table | X[3][N] | red.  The box (exact minimum and maximum of every
// masked position), the masked bandwidth, and L_aa by ov_cross in the shape nbp_overlap_kernel calls it in: the same bits.
__global__ void __launch_bounds__(512)
nbp_overlap_prep_kernel(NBP_OVERLAP_PREP_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *X = smem + NBP_EXPTAB, *red = X + 3 * N;
  const double *s = arena + S * slots[blockIdx.x];
  const ov_geom g = ov_geometry(manifolds[blockIdx.x], masks[blockIdx.x]);
  const int c = slot_count(s, N), n = threadIdx.x;
  nbp_exp_tab_init(tab);
  ov_stage(X, s, N, c, g);
  __syncthreads();
  double h0, h1, h2;
  ov_bandwidth(s, N, g, &h0, &h1, &h2);
  const ov_pair p = ov_setup(g.DK, h0, h1, h2, h0, h1, h2);
  const bool mine = n < c;
  const double lo0 = block_min(mine ? X[n] : INFINITY, red), hi0 = block_max(mine ? X[n] : -INFINITY, red);
  double lo1 = 0.0, hi1 = 0.0, lo2 = 0.0, hi2 = 0.0;
  if (g.DK > 1) {  // (block-uniform)
    lo1 = block_min(mine ? X[N + n] : INFINITY, red);
    hi1 = block_max(mine ? X[N + n] : -INFINITY, red);
  }
  if (g.DK > 2) {
    lo2 = block_min(mine ? X[2 * N + n] : INFINITY, red);
    hi2 = block_max(mine ? X[2 * N + n] : -INFINITY, red);
  }
  double laa = 0.0;
  if (p.ok) laa = ov_cross(X, c, X, c, N, g, p, red, tab);
  if (n == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    nbp_overlap_prep *r = prep + blockIdx.x;
    r->lo[0] = lo0;
    r->lo[1] = lo1;
    r->lo[2] = lo2;
    r->hi[0] = hi0;
    r->hi[1] = hi1;
    r->hi[2] = hi2;
    r->h[0] = h0;
    r->h[1] = h1;
    r->h[2] = h2;
    r->laa = p.ok ? laa : nan;
    r->valid = p.ok ? 1 : 0;
    r->count = c;
  }
}

// the box rule on one Euclidean position: skipped iff gap > 0 and gap^2 > reach^2 (h_i^2 + h_j^2); no square root, one rounding per
// operation (the host restatement makes the same decisions)
__device__ __forceinline__ bool ov_axis_apart(double loi, double hii, double hi_, double loj, double hij, double hj, double reach2) {
  const double gap = fmax(loi - hij, loj - hii);
  return gap > 0.0 && gap * gap > reach2 * (hi_ * hi_ + hj * hj);
}

// One workgroup per row, the same lanes.  LDS: exp table | R[3][N] | P[3][N] | red | top values | top indices | survivors | wave
// counts.  The row's points stay in R.  Partners are taken in runs of one per lane: the box tests, then the survivors of the run
// compacted in index order (ballots and the waves' counts: no atomics, no order-dependent append); each survivor is staged into P
// and evaluated by the whole workgroup with ov_cross, the lanes owning the points of the belief with the LOWER list index -- the
// pair form's value of that pair, bit for bit, in whichever row it is met.  Lane 0 keeps the sorted top-k.  The result is a
// function of the inputs alone.
__global__ void __launch_bounds__(512)
nbp_overlap_search_kernel(NBP_OVERLAP_SEARCH_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *R = smem + NBP_EXPTAB, *P = R + 3 * N, *red = P + 3 * N, *topv = red + NBP_RED;
  int32_t *topi = (int32_t *)(topv + NBP_OVERLAP_MAXK), *surv = topi + NBP_OVERLAP_MAXK, *wcnt = surv + 512;
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (blockDim.x + 63) >> 6;
  const nbp_overlap_prep pi = prep[i];
  int32_t *oi = idx_out + (size_t)i * topk;
  double *ov = logc_out + (size_t)i * topk;
  if (!pi.valid) {  // (block-uniform) a belief with an unusable bandwidth: nobody's partner, and no row of its own
    if (t < topk) {
      oi[t] = -1;
      ov[t] = -INFINITY;
    }
    if (t == 0) {
      found_out[i] = -1;
      evaluated_out[i] = 0;
    }
    return;
  }
  const double *si = arena + S * slots[i];
  const ov_geom g = ov_geometry(manifolds[i], masks[i]);
  nbp_exp_tab_init(tab);
  ov_stage(R, si, N, pi.count, g);
  if (t < NBP_OVERLAP_MAXK) {
    topv[t] = -INFINITY;
    topi[t] = -1;
  }
  __syncthreads();
  int n_found = 0, n_eval = 0;  // (the same in every lane: what they count is block-uniform)
  for (int j0 = 0; j0 < V; j0 += blockDim.x) {
    const int j = j0 + t;
    bool keep = j < V && j != i;
    if (keep) {
      const nbp_overlap_prep *pj = prep + j;
      keep = pj->valid != 0;
      if (keep && !g.c0) keep = !ov_axis_apart(pi.lo[0], pi.hi[0], pi.h[0], pj->lo[0], pj->hi[0], pj->h[0], reach2);
      if (keep && g.DK > 1 && !g.c1) keep = !ov_axis_apart(pi.lo[1], pi.hi[1], pi.h[1], pj->lo[1], pj->hi[1], pj->h[1], reach2);
      if (keep && g.DK > 2 && !g.c2) keep = !ov_axis_apart(pi.lo[2], pi.hi[2], pi.h[2], pj->lo[2], pj->hi[2], pj->h[2], reach2);
    }
    const unsigned long long bal = __ballot(keep);
    __syncthreads();  // (the readers of the previous run's survivors and counts)
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < nw; k++) {
      const int ck = wcnt[k];
      if (k < w) before += ck;
      total += ck;
    }
    if (keep) surv[before + __popcll(bal & ((1ull << lane) - 1ull))] = j;
    __syncthreads();
    for (int q = 0; q < total; q++) {
      const int j2 = surv[q];
      const nbp_overlap_prep pj = prep[j2];
      const ov_geom gj = ov_geometry(manifolds[j2], masks[j2]);
      // (every lane is past the scans of the previous survivor: ov_cross ends in block_sum)
      ov_stage(P, arena + S * slots[j2], N, pj.count, gj);
      __syncthreads();
      double lab;
      if (i < j2) {
        const ov_pair p = ov_setup(g.DK, pi.h[0], pi.h[1], pi.h[2], pj.h[0], pj.h[1], pj.h[2]);
        lab = ov_cross(R, pi.count, P, pj.count, N, g, p, red, tab);
      } else {
        const ov_pair p = ov_setup(g.DK, pj.h[0], pj.h[1], pj.h[2], pi.h[0], pi.h[1], pi.h[2]);
        lab = ov_cross(P, pj.count, R, pi.count, N, g, p, red, tab);
      }
      const double logc = i < j2 ? lab - 0.5 * (pi.laa + pj.laa) : lab - 0.5 * (pj.laa + pi.laa);
      n_eval++;
      if (logc >= logmin) {
        n_found++;
        if (t == 0) {  // descending logc, ties to the lower list index
          int at = topk;
          for (int k = topk - 1; k >= 0; k--)
            if (logc > topv[k] || (logc == topv[k] && (topi[k] < 0 || j2 < topi[k]))) at = k;
          for (int k = topk - 1; k > at; k--) {
            topv[k] = topv[k - 1];
            topi[k] = topi[k - 1];
          }
          if (at < topk) {
            topv[at] = logc;
            topi[at] = j2;
          }
        }
      }
    }
  }
  __syncthreads();
  if (t < topk) {
    oi[t] = topi[t];
    ov[t] = topv[t];
  }
  if (t == 0) {
    found_out[i] = n_found;
    evaluated_out[i] = n_eval;
  }
}
#else
__global__ void nbp_overlap_kernel(NBP_OVERLAP_ARGS);
__global__ void nbp_overlap_prep_kernel(NBP_OVERLAP_PREP_ARGS);
__global__ void nbp_overlap_search_kernel(NBP_OVERLAP_SEARCH_ARGS);
#endif

static inline size_t nbp_overlap_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 6 * (size_t)N + NBP_RED) * 8; }
static inline size_t nbp_overlap_prep_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 3 * (size_t)N + NBP_RED) * 8; }
static inline size_t nbp_overlap_search_lds_bytes(int N) {
  return ((size_t)NBP_EXPTAB + 6 * (size_t)N + NBP_RED + NBP_OVERLAP_MAXK) * 8 + ((size_t)NBP_OVERLAP_MAXK + 512 + 8) * 4;
}
