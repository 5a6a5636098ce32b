// nbp_scene.h -- scene densities: any number of resident beliefs added onto ONE regular 1-D or 2-D grid, the picture of a whole
// solution.  DESIGN.md 3 ("Scene densities") and include/nbp.h hold the definition.  Belief v of the list: slot, manifold, one or
// two coordinates dims_v (all beliefs as many, axis by axis of the same kind: the overlap search's admissibility), weight w_v.
//   usable    the bandwidth entries on dims_v are positive and finite; an unusable belief adds nothing and is reported
//   box       per axis a, d = dims_v[a], h = bw_v[d], mn / mx the exact minimum / maximum of the belief's points on d:
//             cull_lo = mn - reach h, cull_hi = mx + reach h, ext_lo = mn - margin h, ext_hi = mx + margin h, as written
//   grid      point k of axis a = lo_a + (double)k step_a, row-major, axis 0 slowest.  NBP_SCENE_AUTO_EXTENT: Euclidean axis lo = the
//             minimum of ext_lo over the usable beliefs, hi = the maximum of ext_hi, step = (hi - lo) / (n - 1) (no usable belief:
//             lo = step = 0); circular axis lo = -pi, step = 2 pi / n.  Minimum and maximum are order-free.
//   in reach  belief v is in reach of a grid point when cull_lo <= g <= cull_hi on every Euclidean axis; circular axes never cull;
//             reach = +inf puts every belief in reach of every point
//   value     S[k0][k1] = sum_v w_v (P_v / norm_v) over the usable beliefs in reach of the point, in list order; P_v = sum_{j < c_v}
//             E_0[k0][j] E_1[k1][j], j ascending in one lane, E and norm_v those of nbp_marginal_grid_kernel (grid_axis_term; the norm
//             in ascending coordinate order).  One rounding of the division, one of the product with w_v, one of the addition.  A
//             point no belief reaches is exactly 0.0.  A value depends on the list, the weights and its grid point alone.
//   owner     the list index of the largest term w_v (P_v / norm_v) > 0 among the beliefs in reach, ties to the lower index; -1: none
//   bound     a belief out of reach of a point has every particle further than reach h from it on some axis: the term left out is
//             below w_v exp(-reach^2 / 2) / prod_a (sqrt(2 pi) h_a)
// With w = 1, reach = +inf and one belief the grid is nbp_marginal_grid_kernel's bit for bit: the same chunks, the same order, and
// 0.0 + x, 1.0 x are exact.  No floating-point atomics: the order of addition is the list's.
#pragma once
#include "nbp_marginal.h"

// what nbp_scene_prep_kernel leaves per listed belief
struct nbp_scene_rec {
  double cull_lo[2], cull_hi[2], ext_lo[2], ext_hi[2];
  double norm, r[2];  // the marginal kernel's normalisation and 1 / h per axis
  int32_t count, usable;
};

#define NBP_SCENE_PREP_ARGS                                                                                              \
  const int32_t *slots, const int32_t *manifolds, const int32_t *dims, const double *arena, int N, int64_t S, double margin, \
      double reach, nbp_scene_rec *recs, int32_t *skipped
// circ: bit a = axis a is circular; n0, n1: the grid's sizes; extent: lo0, step0, lo1, step1
#define NBP_SCENE_EXTENT_ARGS const nbp_scene_rec *recs, int V, int two, int circ, int n0, int n1, double *extent
// weights: nullable; tile_beliefs: one count per workgroup; owner: read by the owner instance only
#define NBP_SCENE_GRID_ARGS                                                                                              \
  const nbp_scene_rec *recs, const int32_t *slots, const int32_t *dims, const double *weights, int V, const double *arena, \
      int N, int64_t S, int two, int circ, int n0, int n1, const double *extent, double *out, int32_t *owner, int32_t *tile_beliefs
#if NBP_TU & NBP_TU_SCENE
// One workgroup per belief, 64 ceil(N / 64) lanes, lane j brings point j.  The exact minimum and maximum per axis (block_min /
// block_max, as nbp_overlap_prep_kernel), the boxes, the norm in ascending coordinate order, the reciprocals.
__global__ void __launch_bounds__(512)
nbp_scene_prep_kernel(NBP_SCENE_PREP_ARGS) {
  __shared__ double red[NBP_RED];
  const int v = blockIdx.x, t = threadIdx.x;
  const double *s = arena + S * slots[v];
  const int d0 = dims[2 * v], d1 = dims[2 * v + 1];
  const bool two = d1 >= 0;  // (block-uniform)
  const int c = slot_count(s, N);
  const bool mine = t < c;
  const double h0 = s[3 * N + d0], h1 = two ? s[3 * N + d1] : 1.0;
  const double x = mine ? s[d0 * N + t] : 0.0;
  const double mn0 = block_min(mine ? x : INFINITY, red), mx0 = block_max(mine ? x : -INFINITY, red);
  double mn1 = 0.0, mx1 = 0.0;
  if (two) {
    const double y = mine ? s[d1 * N + t] : 0.0;
    mn1 = block_min(mine ? y : INFINITY, red);
    mx1 = block_max(mine ? y : -INFINITY, red);
  }
  if (t == 0) {
    nbp_scene_rec *r = recs + v;
    r->cull_lo[0] = mn0 - reach * h0;
    r->cull_hi[0] = mx0 + reach * h0;
    r->ext_lo[0] = mn0 - margin * h0;
    r->ext_hi[0] = mx0 + margin * h0;
    r->cull_lo[1] = two ? mn1 - reach * h1 : 0.0;
    r->cull_hi[1] = two ? mx1 + reach * h1 : 0.0;
    r->ext_lo[1] = two ? mn1 - margin * h1 : 0.0;
    r->ext_hi[1] = two ? mx1 + margin * h1 : 0.0;
    double norm = (double)c;  // the marginal kernel's order: ascending coordinates
    if (!two) {
      norm *= NBP_SQRT_2PI * h0;
    } else {
      norm *= NBP_SQRT_2PI * (d0 < d1 ? h0 : h1);
      norm *= NBP_SQRT_2PI * (d0 < d1 ? h1 : h0);
    }
    r->norm = norm;
    r->r[0] = 1.0 / h0;
    r->r[1] = 1.0 / h1;
    r->count = c;
    const bool ok = kde_bw_ok(h0) & kde_bw_ok(h1);
    r->usable = ok ? 1 : 0;
    skipped[v] = ok ? 0 : 1;
  }
}

// One workgroup of one wave: the automatic extent of the scene from the records, four doubles.
__global__ void __launch_bounds__(NBP_GRID_LANES)
nbp_scene_extent_kernel(NBP_SCENE_EXTENT_ARGS) {
  const int t = threadIdx.x;
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  int any = 0;
  for (int v = t; v < V; v += NBP_GRID_LANES) {
    const nbp_scene_rec *r = recs + v;
    if (!r->usable) continue;
    any = 1;
    for (int a = 0; a < 2; a++) {
      lo[a] = fmin(lo[a], r->ext_lo[a]);
      hi[a] = fmax(hi[a], r->ext_hi[a]);
    }
  }
  const bool some = __ballot(any) != 0ull;
  for (int a = 0; a < 2; a++) {
    const double l = wave_min(lo[a]), u = wave_max(hi[a]);
    const int n = a ? n1 : n0;
    double o = 0.0, st = 0.0;
    if (a == 0 || two) {
      if (circ >> a & 1) {
        o = -NBP_PI;
        st = NBP_TWO_PI / (double)n;
      } else if (some) {
        o = l;
        st = (u - l) / (double)(n - 1);
      }
    }
    if (t == 0) {
      extent[2 * a] = o;
      extent[2 * a + 1] = st;
    }
  }
}

// whether the tile's span [a, b] of one Euclidean axis meets the record's cull box: a superset of the per-point rule
__device__ __forceinline__ bool scene_span_hit(double a, double b, double cl, double ch) { return cl <= b && a <= ch; }
__device__ __forceinline__ bool scene_in_reach(double g, double cl, double ch) { return cl <= g && g <= ch; }

// One workgroup (one wave) per tile: 32 x 32 points in 2-D in the marginal kernel's lane layout (4 x 4 points per lane), 64 points in
// 1-D.  LDS: exp table | X[2][CHUNK] | E[2][CHUNK][TILE], the marginal kernel's.  The wave walks the records 64 at a time, one per
// lane: each lane tests the tile's span against its record's cull box, a ballot collects the hits, and the hits are taken in
// ascending index order -- no per-tile list in memory.  For a hit the marginal kernel's chunked fill computes E, with 0 where that
// axis point is out of reach: P = 0 exactly at a point the belief does not reach, so the per-point rule costs nothing in the inner
// loop (S + 0.0 = S: the sums are non-negative).  The lane adds w (P / norm) to its 16 sums; OWNER: and keeps the largest term.
template <bool OWNER>
__device__ __forceinline__ void scene_grid_body(NBP_SCENE_GRID_ARGS) {
  __shared__ double tab[NBP_EXPTAB];
  __shared__ double XS[2][NBP_GRID_CHUNK];
  __shared__ double E[2][NBP_GRID_CHUNK][NBP_GRID_TILE];
  const int t = threadIdx.x;
  const bool circ0 = circ & 1, circ1 = (circ >> 1) & 1;
  const double lo0 = extent[0], st0 = extent[1], lo1 = extent[2], st1 = extent[3];
  nbp_exp_tab_init(tab);
  int n_hit = 0;
  if (!two) {
    const int o0 = blockIdx.x * NBP_GRID_TILE1, k = o0 + t;
    const double gk = lo0 + (double)k * st0;
    const double ga = lo0 + (double)o0 * st0, gb = lo0 + (double)min(o0 + NBP_GRID_TILE1 - 1, n0 - 1) * st0;
    const double sa = fmin(ga, gb), sb = fmax(ga, gb);
    double *X = &XS[0][0];
    double sum = 0.0, best = 0.0;
    int own = -1;
    for (int v0 = 0; v0 < V; v0 += NBP_GRID_LANES) {
      const int vl = v0 + t;
      bool hit = false;
      if (vl < V) {
        const nbp_scene_rec *r = recs + vl;
        hit = r->usable != 0 && (circ0 || scene_span_hit(sa, sb, r->cull_lo[0], r->cull_hi[0]));
      }
      unsigned long long bal = __ballot(hit);
      while (bal) {
        const int v = v0 + __ffsll((long long)bal) - 1;
        bal &= bal - 1ull;
        n_hit++;
        const nbp_scene_rec *r = recs + v;
        const double *s = arena + S * slots[v];
        const int d0 = dims[2 * v], c = r->count;
        const double r0 = r->r[0], norm = r->norm, w = weights ? weights[v] : 1.0;
        const bool in = circ0 || scene_in_reach(gk, r->cull_lo[0], r->cull_hi[0]);
        double p = 0.0;
        for (int j0 = 0; j0 < c; j0 += NBP_GRID_TILE1) {
          const int cl = min(NBP_GRID_TILE1, c - j0);
          __syncthreads();  // (the table on the first pass; the readers of the previous chunk afterwards)
          if (t < cl) X[t] = s[d0 * N + j0 + t];
          __syncthreads();
          for (int j = 0; j < cl; j++) p += grid_axis_term(gk, X[j], circ0, r0, tab);
        }
        const double term = w * ((in ? p : 0.0) / norm);
        sum += term;
        if constexpr (OWNER) if (term > best) {
          best = term;
          own = v;
        }
      }
    }
    if (k < n0) {
      out[k] = sum;
      if constexpr (OWNER) owner[k] = own;
    }
    if (t == 0) tile_beliefs[blockIdx.x] = n_hit;
    return;
  }
  const int tiles1 = (n1 + NBP_GRID_TILE - 1) / NBP_GRID_TILE;
  const int o0 = (blockIdx.x / tiles1) * NBP_GRID_TILE, o1 = (blockIdx.x % tiles1) * NBP_GRID_TILE;
  const int lx = t & 7, ly = t >> 3;  // lx along axis 1 (the fastest index of the output), ly along axis 0
  // the fill: lane t computes tile point t & 31 of both axes for the particles (t >> 5), (t >> 5) + 2, .. of the chunk
  const int fk = t & (NBP_GRID_TILE - 1), fj = t >> 5;
  const double g0 = lo0 + (double)(o0 + fk) * st0, g1 = lo1 + (double)(o1 + fk) * st1;
  const double a0 = lo0 + (double)o0 * st0, b0 = lo0 + (double)min(o0 + NBP_GRID_TILE - 1, n0 - 1) * st0;
  const double a1 = lo1 + (double)o1 * st1, b1 = lo1 + (double)min(o1 + NBP_GRID_TILE - 1, n1 - 1) * st1;
  const double sa0 = fmin(a0, b0), sb0 = fmax(a0, b0), sa1 = fmin(a1, b1), sb1 = fmax(a1, b1);
  double sum[NBP_GRID_RB][NBP_GRID_RB], best[OWNER ? NBP_GRID_RB : 1][OWNER ? NBP_GRID_RB : 1];
  int own[OWNER ? NBP_GRID_RB : 1][OWNER ? NBP_GRID_RB : 1];
  for (int a = 0; a < NBP_GRID_RB; a++)
    for (int b = 0; b < NBP_GRID_RB; b++) {
      sum[a][b] = 0.0;
      if constexpr (OWNER) {
        best[a][b] = 0.0;
        own[a][b] = -1;
      }
    }
  for (int v0 = 0; v0 < V; v0 += NBP_GRID_LANES) {
    const int vl = v0 + t;
    bool hit = false;
    if (vl < V) {
      const nbp_scene_rec *r = recs + vl;
      hit = r->usable != 0 && (circ0 || scene_span_hit(sa0, sb0, r->cull_lo[0], r->cull_hi[0])) &&
            (circ1 || scene_span_hit(sa1, sb1, r->cull_lo[1], r->cull_hi[1]));
    }
    unsigned long long bal = __ballot(hit);
    while (bal) {
      const int v = v0 + __ffsll((long long)bal) - 1;  // (wave-uniform)
      bal &= bal - 1ull;
      n_hit++;
      const nbp_scene_rec *r = recs + v;
      const double *s = arena + S * slots[v];
      const int d0 = dims[2 * v], d1 = dims[2 * v + 1], c = r->count;
      const double r0 = r->r[0], r1 = r->r[1], norm = r->norm, w = weights ? weights[v] : 1.0;
      const bool in0 = circ0 || scene_in_reach(g0, r->cull_lo[0], r->cull_hi[0]);
      const bool in1 = circ1 || scene_in_reach(g1, r->cull_lo[1], r->cull_hi[1]);
      double acc[NBP_GRID_RB][NBP_GRID_RB];
      for (int a = 0; a < NBP_GRID_RB; a++)
        for (int b = 0; b < NBP_GRID_RB; b++) acc[a][b] = 0.0;
      for (int j0 = 0; j0 < c; j0 += NBP_GRID_CHUNK) {
        const int cl = min(NBP_GRID_CHUNK, c - j0);
        __syncthreads();  // (the table on the first pass; the readers of the previous chunk afterwards)
        if (fk < cl) XS[fj][fk] = s[(fj ? d1 : d0) * N + j0 + fk];
        __syncthreads();
        for (int j = fj; j < cl; j += 2) {
          const double e0 = grid_axis_term(g0, XS[0][j], circ0, r0, tab), e1 = grid_axis_term(g1, XS[1][j], circ1, r1, tab);
          E[0][j][fk] = in0 ? e0 : 0.0;
          E[1][j][fk] = in1 ? e1 : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cl; j++) {
          double e0[NBP_GRID_RB], e1[NBP_GRID_RB];
          for (int a = 0; a < NBP_GRID_RB; a++) e0[a] = E[0][j][NBP_GRID_RB * ly + a];
          for (int b = 0; b < NBP_GRID_RB; b++) e1[b] = E[1][j][NBP_GRID_RB * lx + b];
          for (int a = 0; a < NBP_GRID_RB; a++)
            for (int b = 0; b < NBP_GRID_RB; b++) acc[a][b] += e0[a] * e1[b];
        }
      }
      for (int a = 0; a < NBP_GRID_RB; a++)
        for (int b = 0; b < NBP_GRID_RB; b++) {
          const double term = w * (acc[a][b] / norm);
          sum[a][b] += term;
          if constexpr (OWNER) if (term > best[a][b]) {
            best[a][b] = term;
            own[a][b] = v;
          }
        }
    }
  }
  for (int a = 0; a < NBP_GRID_RB; a++)
    for (int b = 0; b < NBP_GRID_RB; b++) {
      const int k0 = o0 + NBP_GRID_RB * ly + a, k1 = o1 + NBP_GRID_RB * lx + b;
      if (k0 < n0 && k1 < n1) {
        out[(size_t)k0 * n1 + k1] = sum[a][b];
        if constexpr (OWNER) owner[(size_t)k0 * n1 + k1] = own[a][b];
      }
    }
  if (t == 0) tile_beliefs[blockIdx.x] = n_hit;
}

// two instances: a caller who does not ask for the owner does not pay its registers
__global__ void __launch_bounds__(NBP_GRID_LANES)
nbp_scene_grid_kernel(NBP_SCENE_GRID_ARGS) {
  scene_grid_body<false>(recs, slots, dims, weights, V, arena, N, S, two, circ, n0, n1, extent, out, owner, tile_beliefs);
}
__global__ void __launch_bounds__(NBP_GRID_LANES)
nbp_scene_grid_owner_kernel(NBP_SCENE_GRID_ARGS) {
  scene_grid_body<true>(recs, slots, dims, weights, V, arena, N, S, two, circ, n0, n1, extent, out, owner, tile_beliefs);
}
#else
__global__ void nbp_scene_prep_kernel(NBP_SCENE_PREP_ARGS);
__global__ void nbp_scene_extent_kernel(NBP_SCENE_EXTENT_ARGS);
__global__ void nbp_scene_grid_kernel(NBP_SCENE_GRID_ARGS);
__global__ void nbp_scene_grid_owner_kernel(NBP_SCENE_GRID_ARGS);
#endif
