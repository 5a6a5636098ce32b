// nbp_productgrid.h -- local products on a grid: the product of the messages a variable's factors send it, with the variable's own
// particles replaced by a regular grid over its coordinates.  DESIGN.md 3 ("Local products on a grid") and include/nbp.h hold the
// definition:
//   cell      x = (lo[a] + (double)k_a step[a])_a, one axis per coordinate of the manifold, row-major, coordinate 0 slowest
//   e_jc(x)   the e_ijc of nbp_likelihood.h (lik_term, lik_component: the same bits) with x in role a and u_j in role b (role 0), or
//             u_j in role a and x in role b (role 1); u the resident cloud of the other variable; a unary item: e_c(x) alone
//   log m(x)  M = max_{j,c} e_jc;  S_c = sum_j exp(e_jc - M), j ascending, a term below exp(-700) dropped;  S = sum_c S_c, c ascending;
//             (M + log S) - log n;  M = -inf: -inf.  Both passes in the lane that owns the cell.
//   group     t_k = log_prior_k + log m_k(x); one item: l_g = t_0; more: the running max-shift of include/nbp.h in item order
//   L(x)      sum_g l_g(x) in list order from 0.0
//   record    logmax, argmax (lowest index among equals), logZ = (logmax + log sum exp(L - logmax)) + sum_a log step[a]
// Three kernels: the extents (one wave per grid; the automatic axes are grid_auto_axis of nbp_marginal.h over exact minima and
// maxima, so they are nbp_marginal_grid_kernel's bit for bit), the cells (one workgroup per chunk of 256 consecutive cells of one
// grid, one cell per lane), the normalisation (one workgroup per grid).  No atomics, no block reductions in the fill.
#pragma once
#include "nbp_likelihood.h"
#include "nbp_marginal.h"  // grid_auto_axis

#define NBP_PGRID_EXTENT_ARGS const nbp_product_grid_desc *descs, const double *arena, int N, int64_t S, double *ext
// chunks: (grid, first cell) two ints per workgroup, built by the host; first: the offset of every grid in out; ext: six doubles per
// grid (lo, step per axis) as nbp_product_extent_kernel left them
#define NBP_PGRID_FILL_ARGS                                                                                                        \
  const nbp_product_grid_desc *descs, const nbp_product_item *items, const int32_t *first, const int32_t *chunks, const double *ext, \
      const double *arena, int N, int64_t S, double *out
#define NBP_PGRID_NORM_ARGS \
  const nbp_product_grid_desc *descs, const int32_t *first, const double *ext, const double *logp, nbp_product_grid_rec *recs
#if NBP_TU & NBP_TU_PRODUCTGRID
// One wave per grid: the extent as used, explicit or automatic.  Axes beyond the manifold's coordinates: 0, 0.
__global__ void __launch_bounds__(64)
nbp_product_extent_kernel(NBP_PGRID_EXTENT_ARGS) {
  const nbp_product_grid_desc *g = descs + blockIdx.x;
  const int M = g->manifold, D = mani_dim(M), t = threadIdx.x;
  const bool autoext = g->flags & NBP_PGRID_AUTO_EXTENT;  // (block-uniform)
  const double *s = arena + S * (autoext ? g->slot : 0);
  const int c = autoext ? slot_count(s, N) : 0;
  for (int a = 0; a < 3; a++) {
    double lo = 0.0, st = 0.0;
    if (a < D) {
      lo = g->lo[a];
      st = g->step[a];
      if (autoext) {
        double mn = INFINITY, mx = -INFINITY;
        for (int j = t; j < c; j += 64) {
          const double x = s[a * N + j];
          mn = fmin(mn, x);
          mx = fmax(mx, x);
        }
        grid_auto_axis(is_circ(M, a), wave_min(mn), wave_max(mx), s[3 * N + a], g->margin, g->n[a], &lo, &st);
      }
    }
    if (t == 0) {
      ext[6 * blockIdx.x + 2 * a] = lo;
      ext[6 * blockIdx.x + 2 * a + 1] = st;
    }
  }
}

// what the cell and the staged cloud bring to the pair loop
struct pg_cell {
  double x0, x1, x2;
  const double *B, *SC;  // LDS: the other cloud [3][N]; (sin, cos)[2][N] of its headings where it fills role a of an SE(2) item
  int N, cb;
};

// one pass of the lane over j = 0 .. cb - 1 for one component: PASS 0 the maximum of e, PASS 1 the sum of exp(e - M).  ROLE 0: the
// lane's point is a (l carries it), u_j is b.  ROLE 1: u_j is a, the lane's point b.  Every lane of a wave reads the same LDS address.
template <int KIND, int ZD, int FAM, int ROLE, int PASS>
__device__ __forceinline__ double pg_scan(lik_lane l, const lik_comp &k, const pg_cell &q, double M, const double *tab) {
  double acc = PASS ? 0.0 : -INFINITY;
  const int N = q.N;
  for (int j = 0; j < q.cb; j++) {
    double e;
    if (KIND == NBP_F_PRIOR) {
      e = lik_term<KIND, ZD, FAM>(l, k, 0.0, 0.0, 0.0);
    } else if (ROLE == 0) {
      const double b0 = q.B[j], b1 = l.D > 1 ? q.B[N + j] : 0.0, b2 = l.D > 2 ? q.B[2 * N + j] : 0.0;
      e = lik_term<KIND, ZD, FAM>(l, k, b0, b1, b2);
    } else {
      l.a0 = q.B[j];
      l.a1 = l.D > 1 ? q.B[N + j] : 0.0;
      l.a2 = l.D > 2 ? q.B[2 * N + j] : 0.0;
      if (KIND == NBP_F_SE2) {
        l.sn = q.SC[j];
        l.cs = q.SC[N + j];
      }
      e = lik_term<KIND, ZD, FAM>(l, k, q.x0, q.x1, q.x2);
    }
    if (PASS) {
      const double d = e - M;
      acc += d >= -700.0 ? exp_nonpos(d, tab) : 0.0;  // (-inf and NaN fail the comparison as well)
    } else
      acc = fmax(acc, e);
  }
  return acc;
}

// kind, measurement dimension, family and role are block-uniform runtime values: one dispatch per component and pass, outside the
// pair loop (lik_scan_kind's scheme with the role added; a prior has role 0 only)
template <int KIND, int ZD, int FAM, int PASS>
__device__ __forceinline__ double pg_scan_role(int role, const lik_lane &l, const lik_comp &k, const pg_cell &q, double M, const double *tab) {
  if (KIND != NBP_F_PRIOR && role == 1) return pg_scan<KIND, ZD, FAM, 1, PASS>(l, k, q, M, tab);
  return pg_scan<KIND, ZD, FAM, 0, PASS>(l, k, q, M, tab);
}
template <int KIND, int ZD, int PASS>
__device__ __forceinline__ double pg_scan_fam(int fam, int role, const lik_lane &l, const lik_comp &k, const pg_cell &q, double M,
                                              const double *tab) {
  if (ZD == 1 && fam == NBP_DIST_UNIFORM) return pg_scan_role<KIND, ZD, NBP_DIST_UNIFORM, PASS>(role, l, k, q, M, tab);
  if (ZD == 1 && fam == NBP_DIST_RAYLEIGH) return pg_scan_role<KIND, ZD, NBP_DIST_RAYLEIGH, PASS>(role, l, k, q, M, tab);
  return pg_scan_role<KIND, ZD, NBP_DIST_GAUSSIAN, PASS>(role, l, k, q, M, tab);
}
template <int KIND, int PASS>
__device__ __forceinline__ double pg_scan_zd(int zd, int fam, int role, const lik_lane &l, const lik_comp &k, const pg_cell &q, double M,
                                             const double *tab) {
  if (KIND == NBP_F_CIRCULAR || KIND == NBP_F_EUCLIDDIST || zd == 1) return pg_scan_fam<KIND, 1, PASS>(fam, role, l, k, q, M, tab);
  if (zd == 2) return pg_scan_fam<KIND, 2, PASS>(fam, role, l, k, q, M, tab);
  return pg_scan_fam<KIND, 3, PASS>(fam, role, l, k, q, M, tab);
}
template <int PASS>
__device__ __forceinline__ double pg_scan_kind(int kind, int zd, int fam, int role, const lik_lane &l, const lik_comp &k, const pg_cell &q,
                                               double M, const double *tab) {
  switch (kind) {
    case NBP_F_PRIOR: return pg_scan_zd<NBP_F_PRIOR, PASS>(zd, fam, role, l, k, q, M, tab);
    case NBP_F_LINREL: return pg_scan_zd<NBP_F_LINREL, PASS>(zd, fam, role, l, k, q, M, tab);
    case NBP_F_CIRCULAR: return pg_scan_zd<NBP_F_CIRCULAR, PASS>(zd, fam, role, l, k, q, M, tab);
    case NBP_F_SE2: return pg_scan_zd<NBP_F_SE2, PASS>(zd, fam, role, l, k, q, M, tab);
    default: return pg_scan_zd<NBP_F_EUCLIDDIST, PASS>(zd, fam, role, l, k, q, M, tab);
  }
}

// One workgroup per chunk of NBP_PGRID_CHUNK consecutive cells of one grid, one cell per lane.  LDS: exp table | B[3][N] | SC[2][N].
// Per item the workgroup stages the other cloud (and the sine and cosine of its headings where it fills role a of an SE(2) item,
// formed once), then every lane runs the two passes over j for its own cell: the lanes never exchange a value.  A lane beyond the
// grid's last cell works on that last cell and writes nothing, so every barrier is met by all.  The host has checked everything.
__global__ void __launch_bounds__(NBP_PGRID_CHUNK)
nbp_product_fill_kernel(NBP_PGRID_FILL_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *B = smem + NBP_EXPTAB, *SC = B + 3 * N;
  const int gi = chunks[2 * blockIdx.x], t = threadIdx.x;
  const nbp_product_grid_desc *g = descs + gi;
  const int M = g->manifold, D = mani_dim(M), n1 = g->n[1], n2 = g->n[2];
  const int total = first[gi + 1] - first[gi], at = chunks[2 * blockIdx.x + 1] + t, cell = min(at, total - 1);
  const double *e6 = ext + 6 * gi;
  pg_cell q;
  q.x0 = e6[0] + (double)(cell / (n1 * n2)) * e6[1];
  q.x1 = e6[2] + (double)((cell / n2) % n1) * e6[3];
  q.x2 = e6[4] + (double)(cell % n2) * e6[5];
  q.B = B;
  q.SC = SC;
  q.N = N;
  nbp_exp_tab_init(tab);
  // the cell's own heading, where it fills role a of an SE(2) item: formed once
  double xs = 0.0, xc = 1.0;
  if (M == NBP_SE2) sincos_fast(q.x2, &xs, &xc);
  const int i0 = g->first_item, i1 = i0 + g->n_items;
  double L = 0.0, gm = -INFINITY, gs = 0.0, t0 = 0.0;
  int gc = 0;
  for (int it = i0; it < i1; it++) {
    const nbp_product_item *pi = items + it;
    const nbp_likelihood_desc *d = &pi->lik;
    const int kind = d->kind, role = pi->role, ncomp = d->ncomp;
    const bool unary = kind == NBP_F_PRIOR;
    const double *so = arena + S * (unary ? 0 : pi->other);
    q.cb = unary ? 1 : slot_count(so, N);
    __syncthreads();  // (the table on the first pass; the readers of the previous item's cloud afterwards)
    if (!unary)
      for (int j = t; j < q.cb; j += NBP_PGRID_CHUNK) {
        for (int k = 0; k < D; k++) B[k * N + j] = so[k * N + j];
        if (kind == NBP_F_SE2 && role == 1) sincos_fast(so[2 * N + j], &SC[j], &SC[N + j]);
      }
    __syncthreads();
    // the coordinates of the measurement, the circular flags: as nbp_likelihood_kernel forms them
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
    l.a0 = q.x0;
    l.a1 = q.x1;
    l.a2 = q.x2;
    l.sn = kind == NBP_F_SE2 ? xs : 0.0;
    l.cs = kind == NBP_F_SE2 ? xc : 1.0;
    double wsum = 0.0;
    for (int c = 0; c < ncomp; c++) wsum += d->comp[c][0];
    // ---- pass 1: the maximum over every neighbour point and component; pass 2: the sums relative to it ----
    double mx = -INFINITY;
    for (int c = 0; c < ncomp; c++) {
      const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
      const lik_comp k = lik_component(d, c, zd, fam, wsum);
      mx = fmax(mx, pg_scan_kind<0>(kind, zd, fam, role, l, k, q, 0.0, tab));
    }
    double logm = -INFINITY;
    if (mx > -INFINITY) {
      double s = 0.0;
      for (int c = 0; c < ncomp; c++) {
        const int fam = zd == 1 ? (int)d->comp[c][12] : NBP_DIST_GAUSSIAN;
        const lik_comp k = lik_component(d, c, zd, fam, wsum);
        s += pg_scan_kind<1>(kind, zd, fam, role, l, k, q, mx, tab);
      }
      logm = (mx + nbpm_log(s)) - nbpm_log((double)q.cb);
    }
    // ---- the group: one item as it is, more by the running max-shift ----
    const double tk = pi->log_prior + logm;
    if (it == i0 || items[it - 1].group != pi->group) {  // (block-uniform)
      gm = -INFINITY;
      gs = 0.0;
      gc = 0;
      t0 = tk;
    }
    gc++;
    if (tk > gm) {
      const double dd = gm - tk;
      gs = (gm > -INFINITY ? gs * (dd >= -700.0 ? exp_nonpos(dd, tab) : 0.0) : 0.0) + 1.0;
      gm = tk;
    } else if (tk > -INFINITY) {
      const double dd = tk - gm;
      gs += dd >= -700.0 ? exp_nonpos(dd, tab) : 0.0;
    }
    if (it == i1 - 1 || items[it + 1].group != pi->group)
      L += gc == 1 ? t0 : (gm > -INFINITY ? gm + nbpm_log(gs) : -INFINITY);
  }
  if (at < total) out[first[gi] + at] = L;
}

// One workgroup per grid: lane t owns the cells t, t + 256, .. in ascending order; the maximum and the lowest index that holds it, the
// sum relative to it (block_sum: a fixed order), the record.
__global__ void __launch_bounds__(NBP_PGRID_CHUNK)
nbp_product_norm_kernel(NBP_PGRID_NORM_ARGS) {
  __shared__ double tab[NBP_EXPTAB];
  __shared__ double red[NBP_RED];
  const nbp_product_grid_desc *g = descs + blockIdx.x;
  const int t = threadIdx.x, total = first[blockIdx.x + 1] - first[blockIdx.x], D = mani_dim(g->manifold);
  const double *L = logp + first[blockIdx.x];
  nbp_exp_tab_init(tab);
  double mx = -INFINITY;
  int ix = 0;
  for (int k = t; k < total; k += NBP_PGRID_CHUNK) {
    const double v = L[k];
    if (v > mx) {
      mx = v;
      ix = k;
    }
  }
  const double Mx = block_max(mx, red);
  const double am = block_min((mx == Mx && Mx > -INFINITY) ? (double)ix : INFINITY, red);  // (cell indices are exact in a double)
  double s = 0.0;
  if (Mx > -INFINITY)  // (block-uniform)
    for (int k = t; k < total; k += NBP_PGRID_CHUNK) {
      const double d = L[k] - Mx;
      s += d >= -700.0 ? exp_nonpos(d, tab) : 0.0;
    }
  const double Z = block_sum(s, red);
  if (t == 0) {
    nbp_product_grid_rec *r = recs + blockIdx.x;
    double lz = -INFINITY;
    if (Mx > -INFINITY) {
      lz = Mx + nbpm_log(Z);
      double ls = 0.0;
      for (int a = 0; a < D; a++)
        if (g->n[a] > 1) ls += nbpm_log(ext[6 * blockIdx.x + 2 * a + 1]);
      lz += ls;
    }
    r->logZ = lz;
    r->logmax = Mx;
    r->argmax = Mx > -INFINITY ? (int32_t)am : -1;
    r->pad = 0;
  }
}
#else
__global__ void nbp_product_extent_kernel(NBP_PGRID_EXTENT_ARGS);
__global__ void nbp_product_fill_kernel(NBP_PGRID_FILL_ARGS);
__global__ void nbp_product_norm_kernel(NBP_PGRID_NORM_ARGS);
#endif

static inline size_t nbp_product_fill_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 5 * (size_t)N) * 8; }
