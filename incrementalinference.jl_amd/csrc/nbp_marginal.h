// nbp_marginal.h -- marginal densities of resident beliefs: on a regular 1-D or 2-D grid over a subset K of the manifold's
// coordinates (the x-y picture of a pose, the 1-D picture of one coordinate) and at arbitrary query points.  DESIGN.md 3 holds
// the definitions; coordinates are tangent coordinates at the identity (SE(2): x, y, theta), as in nbp_query.h.
//   marginal  p_K(q) = 1 / norm * sum_{j < c} exp(e(q, x_j)), e and norm the exponent and the normalisation of nbp_kde.h over the
//             coordinates in K: the density of nbp_query.h with the coordinates outside K dropped (integrating a coordinate out
//             of a product-kernel KDE is dropping it).  Only the bandwidth entries IN K must be positive and finite (else every
//             value is NaN); the others are not read: a partial belief has a marginal.
//   grid      point k of axis a is lo_a + (double)k * step_a; the output is row-major, the first listed coordinate slowest.
//             E_a[k][j] = exp_nonpos(-1/2 (((g_a[k] - x_j[d_a]) wrapped where circular) * (1 / h_a))^2), the per-axis arithmetic
//             of nbp_eval_kernel; 2-D value = (sum_j E_0[k0][j] * E_1[k1][j]) / norm, 1-D value = (sum_j E_0[k0][j]) / norm,
//             j = 0 .. c - 1 in that order in ONE lane, norm = c * prod sqrt(2 pi) h_d over K in ASCENDING coordinate order (the
//             eval kernel's order: dims = (b, a) is the transpose of dims = (a, b) bit for bit).  A value depends on the belief
//             and its grid point alone -- not on the tile, the launch or the descriptors that travel with it.
//   extent    NBP_GRID_AUTO_EXTENT: Euclidean axis lo = min_j x - margin h, hi = max_j x + margin h, step = (hi - lo) / (n - 1);
//             circular axis lo = -pi, step = 2 pi / n.  min and max are exact and order-free, so every workgroup of a descriptor
//             derives the same extent; the workgroup of the tile at the origin writes it out.
// The separable form is the point of the grid kernel: a T x T tile needs 2 T c exponentials, not T^2 c; what remains per
// (grid point, particle) pair is one multiplication and one addition.  DEFINED here, unpinned against KernelDensityEstimate.jl
// (DESIGN.md 8).
#pragma once
#include "nbp_kde.h"
#include "nbp_query.h"  // eval_body

#define NBP_GRID_TILE 32    // 2-D: grid points per axis of one tile
#define NBP_GRID_RB 4       // 2-D: a lane owns RB x RB points of the tile (8 x 8 lanes: one wave per tile)
#define NBP_GRID_CHUNK 32   // 2-D: particles per chunk of the per-axis tables
#define NBP_GRID_TILE1 64   // 1-D: grid points of one tile, one per lane; also its chunk of particles
#define NBP_GRID_LANES 64

// nbp_marginal_grid_kernel -- tiles: (descriptor, k0 origin, k1 origin), three ints each, built by the host; first: the offset of
// every descriptor's grid in out; extent: four doubles per descriptor (lo0, step0, lo1, step1; a 1-D grid: lo1 = step1 = 0).
#define NBP_GRID_ARGS                                                                                                  \
  const nbp_grid_desc *descs, const int32_t *first, const int32_t *tiles, const double *arena, int N, int64_t S,       \
      double *out, double *extent
// nbp_eval_marginal_kernel -- nbp_eval_kernel's arguments and one coordinate bit mask per belief
#define NBP_EVAL_MARGINAL_ARGS                                                                                         \
  const int32_t *tiles, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, const double *arena,     \
      int N, int64_t S, const double *queries, double *dens
#if NBP_TU & (NBP_TU_MARGINAL | NBP_TU_SCENE)
// one entry of a per-axis table (the scene kernels of nbp_scene.h call it too: the same bits)
__device__ __forceinline__ double grid_axis_term(double g, double x, bool circ, double r, const double *tab) {
  double d = g - x;
  if (circ) d = wrap_pi(d);
  d *= r;
  return exp_nonpos(-0.5 * (d * d), tab);
}
#endif
#if NBP_TU & (NBP_TU_MARGINAL | NBP_TU_PRODUCTGRID)
// (the product grids of nbp_productgrid.h take their automatic axes from it too: the same bits)
// the automatic extent of one axis from the exact minimum and maximum of its coordinate
__device__ __forceinline__ void grid_auto_axis(bool circ, double mn, double mx, double h, double margin, int n, double *lo,
                                               double *step) {
  if (circ) {
    *lo = -NBP_PI;
    *step = NBP_TWO_PI / (double)n;
  } else {
    const double l = mn - margin * h, u = mx + margin * h;
    *lo = l;
    *step = (u - l) / (double)(n - 1);
  }
}
#endif
#if NBP_TU & NBP_TU_MARGINAL

// One workgroup (one wave) per tile.  LDS: exp table | X[2][CHUNK] | E[2][CHUNK][TILE].  2-D: over chunks of particles in
// ascending order the wave stages the two coordinate rows, fills E_0[j][k0] and E_1[j][k1] -- one exponential per (axis point,
// particle), shared by the tile; the tile index moves fastest, so the lanes of the wave read consecutive doubles or the same one --
// and lane (ly, lx) adds E_0[j][4 ly + a] * E_1[j][4 lx + b] to its 4 x 4 sums, j ascending: eight LDS doubles per sixteen pairs.
// 1-D: lane t owns point k0 + t and walks j over the staged row (the eval kernel's loop on one coordinate).  No atomics.
__global__ void __launch_bounds__(NBP_GRID_LANES)
nbp_marginal_grid_kernel(NBP_GRID_ARGS) {
  __shared__ double tab[NBP_EXPTAB];
  __shared__ double XS[2][NBP_GRID_CHUNK];
  __shared__ double E[2][NBP_GRID_CHUNK][NBP_GRID_TILE];
  static_assert(2 * NBP_GRID_CHUNK >= NBP_GRID_TILE1, "the 1-D path stages its chunk in XS");
  static_assert(NBP_GRID_TILE * 2 == NBP_GRID_LANES && NBP_GRID_TILE == 8 * NBP_GRID_RB, "lane layout of the 2-D path");
  const int t = threadIdx.x, gi = tiles[3 * blockIdx.x], o0 = tiles[3 * blockIdx.x + 1], o1 = tiles[3 * blockIdx.x + 2];
  const nbp_grid_desc *g = descs + gi;
  const double *s = arena + S * g->slot;
  const int M = g->manifold, d0 = g->dims[0], d1 = g->dims[1];
  const bool two = d1 >= 0;  // block-uniform, like everything read from the descriptor
  const int n0 = g->n[0], n1 = two ? g->n[1] : 1;
  const int c = slot_count(s, N);
  nbp_exp_tab_init(tab);
  const double h0 = s[3 * N + d0], h1 = two ? s[3 * N + d1] : 1.0;
  const bool circ0 = is_circ(M, d0), circ1 = two && is_circ(M, d1);
  double lo0 = g->lo[0], st0 = g->step[0], lo1 = two ? g->lo[1] : 0.0, st1 = two ? g->step[1] : 0.0;
  if (g->flags & NBP_GRID_AUTO_EXTENT) {
    double mn0 = INFINITY, mx0 = -INFINITY, mn1 = INFINITY, mx1 = -INFINITY;
    for (int j = t; j < c; j += NBP_GRID_LANES) {
      const double x = s[d0 * N + j];
      mn0 = fmin(mn0, x);
      mx0 = fmax(mx0, x);
      if (two) {
        const double y = s[d1 * N + j];
        mn1 = fmin(mn1, y);
        mx1 = fmax(mx1, y);
      }
    }
    grid_auto_axis(circ0, wave_min(mn0), wave_max(mx0), h0, g->margin, n0, &lo0, &st0);
    if (two) grid_auto_axis(circ1, wave_min(mn1), wave_max(mx1), h1, g->margin, n1, &lo1, &st1);
  }
  if (o0 == 0 && o1 == 0 && t == 0) {
    extent[4 * gi] = lo0;
    extent[4 * gi + 1] = st0;
    extent[4 * gi + 2] = lo1;
    extent[4 * gi + 3] = st1;
  }
  double *o = out + first[gi];
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double norm = (double)c;  // the eval kernel's order: ascending coordinates
  if (!two) {
    norm *= NBP_SQRT_2PI * h0;
  } else {
    norm *= NBP_SQRT_2PI * (d0 < d1 ? h0 : h1);
    norm *= NBP_SQRT_2PI * (d0 < d1 ? h1 : h0);
  }
  if (!two) {
    const int k = o0 + t;
    if (!valid) {
      if (k < n0) o[k] = qnan;
      return;
    }
    const double gk = lo0 + (double)k * st0, r0 = 1.0 / h0;
    double *X = &XS[0][0];
    double p = 0.0;
    for (int j0 = 0; j0 < c; j0 += NBP_GRID_TILE1) {
      const int cl = min(NBP_GRID_TILE1, c - j0);
      __syncthreads();  // (the table on the first pass; the readers of the previous chunk afterwards)
      if (t < cl) X[t] = s[d0 * N + j0 + t];
      __syncthreads();
      for (int j = 0; j < cl; j++) p += grid_axis_term(gk, X[j], circ0, r0, tab);
    }
    if (k < n0) o[k] = p / norm;
    return;
  }
  const int lx = t & 7, ly = t >> 3;  // lx along axis 1 (the fastest index of the output), ly along axis 0
  if (!valid) {
    for (int a = 0; a < NBP_GRID_RB; a++)
      for (int b = 0; b < NBP_GRID_RB; b++) {
        const int k0 = o0 + NBP_GRID_RB * ly + a, k1 = o1 + NBP_GRID_RB * lx + b;
        if (k0 < n0 && k1 < n1) o[(size_t)k0 * n1 + k1] = qnan;
      }
    return;
  }
  // the fill: lane t computes tile point t & 31 of both axes for the particles (t >> 5), (t >> 5) + 2, .. of the chunk
  const int fk = t & (NBP_GRID_TILE - 1), fj = t >> 5;
  const double g0 = lo0 + (double)(o0 + fk) * st0, g1 = lo1 + (double)(o1 + fk) * st1, r0 = 1.0 / h0, r1 = 1.0 / h1;
  double acc[NBP_GRID_RB][NBP_GRID_RB];
  for (int a = 0; a < NBP_GRID_RB; a++)
    for (int b = 0; b < NBP_GRID_RB; b++) acc[a][b] = 0.0;
  for (int j0 = 0; j0 < c; j0 += NBP_GRID_CHUNK) {
    const int cl = min(NBP_GRID_CHUNK, c - j0);
    __syncthreads();  // (the table on the first pass; the readers of the previous chunk afterwards)
    if (fk < cl) XS[fj][fk] = s[(fj ? d1 : d0) * N + j0 + fk];
    __syncthreads();
    for (int j = fj; j < cl; j += 2) {
      E[0][j][fk] = grid_axis_term(g0, XS[0][j], circ0, r0, tab);
      E[1][j][fk] = grid_axis_term(g1, XS[1][j], circ1, r1, tab);
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
      const int k0 = o0 + NBP_GRID_RB * ly + a, k1 = o1 + NBP_GRID_RB * lx + b;
      if (k0 < n0 && k1 < n1) o[(size_t)k0 * n1 + k1] = acc[a][b] / norm;
    }
}

// nbp_eval_kernel's body with the belief's mask in place of the constant 7: one function, so the full mask delivers
// nbp_eval_kernel's values bit for bit.
__global__ void __launch_bounds__(NBP_QUERY_TILE)
nbp_eval_marginal_kernel(NBP_EVAL_MARGINAL_ARGS) {
  eval_body(tiles, slots, manifolds, arena, N, S, queries, dens, masks[tiles[3 * blockIdx.x]]);
}
#else
__global__ void nbp_marginal_grid_kernel(NBP_GRID_ARGS);
__global__ void nbp_eval_marginal_kernel(NBP_EVAL_MARGINAL_ARGS);
#endif
