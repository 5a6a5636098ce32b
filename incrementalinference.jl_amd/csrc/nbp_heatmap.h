// nbp_heatmap.h -- a samplable density from a scalar field on a regular x-y grid: the reference's HeatmapGridDensity /
// LevelSetGridNormal (ext/HeatmapSampler.jl:123-242), built on the device.  DESIGN.md 3 ("Heatmap densities") holds the
// definitions, DESIGN.md 8 the deviations from the reference; heatmap.py restates every line below in numpy.
//
//   field     data[i * ny + j] at (x[i], y[j]), nx, ny >= 2, uniform spacing dx, dy, n = nx * ny <= 2^26 cells.
//   h         bw_factor * 0.5 * (dx + dy), both coordinates (fitKDE, :144-159).
//   cells     w_c = data_c where 0 < data_c, else 0; cdf = SCAN(w); total = cdf[n - 1]  (sampleHeatmap(field, x, y, 0), :123-140).
//   pre       m = 0 .. M-1: (ua, _) = uniform_pair(seed, m, PURP_HMCELL, 0); c = SEARCH(cdf, ua * total), moved on to the next cell
//             with w > 0 should w_c = 0 (the last such cell -- the host finds it while it checks the field -- where none follows);
//             (n0, n1) = normal_pair(seed, m, PURP_HMNOISE, 0); p_m = (x[i] + h * n0, y[j] + h * n1), c = i * ny + j
//             (sample(density_, N), :179).
//   d         hm_bilinear(p_m) inside [x[0], x[nx-1]] x [y[0], y[ny-1]], else 0  (:185-195).
//   W         W_m = exp_nonpos(-(d_m - dmin)), dmin = min_m d_m (exact, order-free); wcdf = SCAN(W); wtotal = wcdf[M - 1]  (:198-199).
//   draw      k = 0 .. n-1: (ua, _) = uniform_pair(seed2, k, PURP_HMPICK, 0); pick = SEARCH(wcdf, ua * wtotal); point = pre[pick],
//             with jitter + h * normal_pair(seed2, k, PURP_HMNOISE, 1); bandwidth (h, h).
//
// SCAN -- the inclusive prefix sum in a FIXED order, a function of the length alone, one rounding per addition:
//   scan(a): cut a into segments of NBP_HM_SEG = 64 consecutive elements (the last may be shorter).  Within a segment run the
//   Kogge-Stone steps o = 1, 2, 4, 8, 16, 32: l[i] <- l[i] + l[i - o] for every i >= o of the segment, all i of a step at once
//   (from the values before the step).  One segment: scan(a) = l.  Else T[s] = l at the LAST element of segment s,
//   P = scan(T) (the same function, on the n / 64 totals), and scan(a)[i] = l[i] + P[s - 1] for i in segment s >= 1,
//   l[i] for segment 0.  Lengths up to 2^26 recurse four times (2^26 -> 2^20 -> 2^14 -> 2^8 -> 4).
//   On the device a segment is one wave (the steps are lane shifts in registers), 64 segments are one workgroup's tile of
//   NBP_HM_TILE = 4096 elements (the scan of its 64 totals: one wave again, through LDS); nbp_hm_scan_totals_kernel reads the
//   input once and leaves the tile totals T2, nbp_hm_scan_tiles_kernel (one workgroup) scans those -- P2 = scan(T2), levels
//   2^14 -> 2^8 -> 4 through LDS --, nbp_hm_scan_apply_kernel reads the input again and writes scan(a): two passes over the
//   input, one write, all of it 8 bytes a lane and consecutive.  A sum is not monotone to the last bit across lanes, so:
// SEARCH(cdf, t) -- binary search (lo, hi -> mid = (lo + hi) >> 1; t < cdf[mid] ? hi = mid : lo = mid + 1; until lo == hi), first
//   over the tiles b with cdf at the tile's last element as the probe, then within the tile found: the first element with
//   t < cdf wherever cdf is monotone; the last element where rounding leaves none.  Nothing is normalised: no division.
#pragma once
#include "nbp_kernels.h"

#define PURP_HMCELL 16        // ua -> the cell of pre-sample m (k = 0)
#define PURP_HMNOISE 17       // kernel noise: k = 0 of a pre-sample (seed), k = 1 of a jittered draw (seed2)
#define PURP_HMPICK 18        // ua -> the pre-sample that draw k takes (k = 0)
#define NBP_HM_SEG 64
#define NBP_HM_TILE 4096
#define NBP_HM_LANES 256      // of every kernel here: four waves; a wave of a scan kernel owns 16 segments of its tile
#define NBP_HM_MAX_CELLS (1 << 26)
#define NBP_HM_MAX_TILES (NBP_HM_MAX_CELLS / NBP_HM_TILE)  // 2^14: what the one workgroup of nbp_hm_scan_tiles_kernel scans

// Bilinear interpolation of the field at (px, py) inside the grid's box; one rounding per written operation (the library is
// compiled without contraction).  The cell by arithmetic on (p - x0) / dx, clamped to nx - 2 / ny - 2 (p on the upper edge: t = 1).
static __host__ __device__ __forceinline__ double hm_bilinear(const double *data, int nx, int ny, double x0, double y0, double dx,
                                                              double dy, double px, double py) {
  const double fx = (px - x0) / dx, fy = (py - y0) / dy;
  int i0 = (int)fx, j0 = (int)fy;
  i0 = i0 > nx - 2 ? nx - 2 : i0;
  j0 = j0 > ny - 2 ? ny - 2 : j0;
  const double tx = fx - (double)i0, ty = fy - (double)j0;
  const double *r0 = data + (size_t)i0 * ny + j0, *r1 = r0 + ny;
  const double a = (1.0 - ty) * r0[0] + ty * r0[1], b = (1.0 - ty) * r1[0] + ty * r1[1];
  return (1.0 - tx) * a + tx * b;
}

#define NBP_HM_TOTALS_ARGS const double *in, int n, double *t2
#define NBP_HM_TILES_ARGS const double *t2, int m, double *p2
#define NBP_HM_APPLY_ARGS const double *in, int n, const double *t2, const double *p2, double *out
#define NBP_HM_PRE_ARGS                                                                                                 \
  const double *data, const double *x, const double *y, const double *cdf, const int *lastpos, int nx, int ny, double dx, \
      double dy, double h, int M, uint64_t seed, int32_t *cell, double2 *pre, double *d, unsigned long long *dmin_key
#define NBP_HM_WEIGHT_ARGS const double *d, const unsigned long long *dmin_key, int M, double *W
#define NBP_HM_DRAW_ARGS                                                                                                \
  const double *wcdf, const double2 *pre, int M, double h, int n, uint64_t seed, int jitter, int32_t *pick, double2 *pts, \
      double *slot, int N
#define NBP_HM_SEARCH_ARGS const double *cdf, int n, const double *t, int nt, int32_t *idx
#if NBP_TU & NBP_TU_HEATMAP
__device__ __forceinline__ double hm_weight(double v) { return v > 0.0 ? v : 0.0; }  // (NaN never arrives: the host refuses it)

// the Kogge-Stone steps of one segment, lane = position in the segment; lanes beyond a short segment carry +0 (x + 0 = x: the
// elements of the segment see the sums of the definition)
__device__ __forceinline__ double hm_wave_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < NBP_HM_SEG; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v = v + u;
  }
  return v;
}

// l of the 16 segments a wave owns in its tile (segment w * 16 + j in l[j]) and the segments' totals in t1[64] (0 for a segment
// beyond the end).  Ends with a barrier.
__device__ __forceinline__ void hm_tile_segments(const double *in, int n, int base, double *t1, double l[16]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int seg = w * 16 + j, i0 = base + seg * NBP_HM_SEG, cnt = min(NBP_HM_SEG, n - i0);  // cnt: wave-uniform
    const double v = lane < cnt ? hm_weight(in[i0 + lane]) : 0.0;
    l[j] = hm_wave_scan(v, lane);
    const double tot = __shfl(l[j], cnt > 0 ? cnt - 1 : 0, 64);
    if (lane == 0) t1[seg] = cnt > 0 ? tot : 0.0;
  }
  __syncthreads();
}

// pass 1: the total of every tile (T2 of the definition: l of the tile's segment totals at the last segment)
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_scan_totals_kernel(NBP_HM_TOTALS_ARGS) {
  __shared__ double t1[NBP_HM_SEG];
  const int lane = threadIdx.x & 63, base = blockIdx.x * NBP_HM_TILE;
  double l[16];
  hm_tile_segments(in, n, base, t1, l);
  if (threadIdx.x < 64) {
    const int nseg = min(NBP_HM_SEG, (n - base + NBP_HM_SEG - 1) / NBP_HM_SEG);
    const double s = hm_wave_scan(lane < nseg ? t1[lane] : 0.0, lane);
    const double tot = __shfl(s, nseg - 1, 64);
    if (lane == 0) t2[blockIdx.x] = tot;
  }
}

// pass 2, one workgroup: P2 = scan(T2) for m <= NBP_HM_MAX_TILES tile totals.  T2 -> l2 (kept in p2) and T3 (LDS, <= 256);
// T3 -> l3 and T4 (<= 4); P4 = l4; P3 = l3 + P4[.]; P2 = l2 + P3[.]
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_scan_tiles_kernel(NBP_HM_TILES_ARGS) {
  __shared__ double t3[256], p3[256], t4[4], p4[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nseg2 = (m + NBP_HM_SEG - 1) / NBP_HM_SEG, nseg3 = (nseg2 + NBP_HM_SEG - 1) / NBP_HM_SEG;
  for (int s2 = w; s2 < nseg2; s2 += NBP_HM_LANES / 64) {
    const int i0 = s2 * NBP_HM_SEG, cnt = min(NBP_HM_SEG, m - i0);
    const double s = hm_wave_scan(lane < cnt ? t2[i0 + lane] : 0.0, lane);
    if (lane < cnt) p2[i0 + lane] = s;
    const double tot = __shfl(s, cnt - 1, 64);
    if (lane == 0) t3[s2] = tot;
  }
  __syncthreads();
  if (w < nseg3) {
    const int i0 = w * NBP_HM_SEG, cnt = min(NBP_HM_SEG, nseg2 - i0);
    const double s = hm_wave_scan(lane < cnt ? t3[i0 + lane] : 0.0, lane);
    if (lane < cnt) p3[i0 + lane] = s;
    const double tot = __shfl(s, cnt - 1, 64);
    if (lane == 0) t4[w] = tot;
  }
  __syncthreads();
  if (w == 0) {
    const double s = hm_wave_scan(lane < nseg3 ? t4[lane] : 0.0, lane);
    if (lane < nseg3) p4[lane] = s;
  }
  __syncthreads();
  const int t = threadIdx.x;  // (nseg2 <= 256: one element of level 3 per lane)
  double v3 = 0.0;
  if (t < nseg2) v3 = t >= NBP_HM_SEG ? p3[t] + p4[t / NBP_HM_SEG - 1] : p3[t];
  __syncthreads();
  if (t < nseg2) p3[t] = v3;
  __syncthreads();
  for (int i = t; i < m; i += NBP_HM_LANES)
    if (i >= NBP_HM_SEG) p2[i] = p2[i] + p3[i / NBP_HM_SEG - 1];
}

// pass 3: scan(a) of the tile.  P1[s] = l1[s] + P2[b - 1] for segment s of tile b >= 1 (l1[s] in tile 0); the elements of
// segment s >= 1 add P1[s - 1] -- for the first segment of a tile that is the last P1 of the tile before, T2[b-1] + P2[b-2].
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_scan_apply_kernel(NBP_HM_APPLY_ARGS) {
  __shared__ double t1[NBP_HM_SEG];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x, base = b * NBP_HM_TILE;
  double l[16];
  hm_tile_segments(in, n, base, t1, l);
  const double l1 = hm_wave_scan(t1[lane], lane);  // every wave for itself (segments beyond the end hold 0)
  const double prev = __shfl_up(l1, 1, 64);
  double carry = 0.0;  // of segment `lane` of this tile; none for the very first segment
  if (lane > 0) carry = b > 0 ? prev + p2[b - 1] : prev;
  else if (b == 1) carry = t2[0];
  else if (b > 1) carry = t2[b - 1] + p2[b - 2];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int seg = w * 16 + j, i = base + seg * NBP_HM_SEG + lane;
    const double c = __shfl(carry, seg, 64);
    if (i < n) out[i] = (b == 0 && seg == 0) ? l[j] : l[j] + c;
  }
}

__device__ __forceinline__ int hm_search(const double *cdf, int n, double t) {
  int lo = 0, hi = (n + NBP_HM_TILE - 1) / NBP_HM_TILE - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < cdf[min((mid + 1) * NBP_HM_TILE, n) - 1]) hi = mid;
    else lo = mid + 1;
  }
  lo = hi * NBP_HM_TILE;
  hi = min(lo + NBP_HM_TILE, n) - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < cdf[mid]) hi = mid;
    else lo = mid + 1;
  }
  return hi;
}

// the total order of finite doubles as unsigned integers (for an exact, order-free minimum by atomicMin)
__device__ __forceinline__ unsigned long long hm_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double hm_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// one lane per pre-sample: cell, point, field value; the minimum of the field values into *dmin_key (preset to all ones)
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_presample_kernel(NBP_HM_PRE_ARGS) {
  const int m = blockIdx.x * NBP_HM_LANES + threadIdx.x, n = nx * ny;
  double dm = INFINITY;
  if (m < M) {
    double ua, ub, n0, n1;
    uniform_pair(seed, (uint32_t)m, PURP_HMCELL, 0, ua, ub);
    int c = hm_search(cdf, n, ua * cdf[n - 1]);
    while (c < n - 1 && !(data[c] > 0.0)) c++;
    if (!(data[c] > 0.0)) c = *lastpos;
    const int i = c / ny, j = c - i * ny;
    normal_pair(seed, (uint32_t)m, PURP_HMNOISE, 0, n0, n1);
    const double px = x[i] + h * n0, py = y[j] + h * n1;
    const double x0 = x[0], y0 = y[0];
    dm = 0.0;
    if (px >= x0 && px <= x[nx - 1] && py >= y0 && py <= y[ny - 1]) dm = hm_bilinear(data, nx, ny, x0, y0, dx, dy, px, py);
    cell[m] = c;
    pre[m] = make_double2(px, py);
    d[m] = dm;
  }
  dm = wave_min(dm);
  if ((threadIdx.x & 63) == 0 && dm < INFINITY) atomicMin(dmin_key, hm_key(dm));
}

__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_weight_kernel(NBP_HM_WEIGHT_ARGS) {
  __shared__ double tab[NBP_EXPTAB];
  nbp_exp_tab_init(tab);
  __syncthreads();
  const int m = blockIdx.x * NBP_HM_LANES + threadIdx.x;
  if (m < M) W[m] = exp_nonpos(-(d[m] - hm_unkey(*dmin_key)), tab);
}

// one lane per drawn point; slot != nullptr: also rows 0 and 1 of the belief slot (zeroed by the host before the launch) and
// its bandwidth (h, h, 0) and count, as pack_belief lays an NBP_EUCLID2 belief of n points out
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_draw_kernel(NBP_HM_DRAW_ARGS) {
  const int k = blockIdx.x * NBP_HM_LANES + threadIdx.x;
  if (k >= n) return;
  double ua, ub;
  uniform_pair(seed, (uint32_t)k, PURP_HMPICK, 0, ua, ub);
  const int p = hm_search(wcdf, M, ua * wcdf[M - 1]);
  double2 q = pre[p];
  if (jitter) {
    double n0, n1;
    normal_pair(seed, (uint32_t)k, PURP_HMNOISE, 1, n0, n1);
    q.x = q.x + h * n0;
    q.y = q.y + h * n1;
  }
  pick[k] = p;
  pts[k] = q;
  if (slot) {
    slot[k] = q.x;
    slot[N + k] = q.y;
    if (k == 0) {
      slot[3 * N] = h;
      slot[3 * N + 1] = h;
      slot[3 * N + 6] = n < N ? (double)n : 0.0;
    }
  }
}

// the self-test of SEARCH (nbp_heatmap_search_eval): one lane per probe, cdf any array of n doubles
__global__ void __launch_bounds__(NBP_HM_LANES)
nbp_hm_search_eval_kernel(NBP_HM_SEARCH_ARGS) {
  const int k = blockIdx.x * NBP_HM_LANES + threadIdx.x;
  if (k < nt) idx[k] = hm_search(cdf, n, t[k]);
}
#else
__global__ void nbp_hm_scan_totals_kernel(NBP_HM_TOTALS_ARGS);
__global__ void nbp_hm_scan_tiles_kernel(NBP_HM_TILES_ARGS);
__global__ void nbp_hm_scan_apply_kernel(NBP_HM_APPLY_ARGS);
__global__ void nbp_hm_presample_kernel(NBP_HM_PRE_ARGS);
__global__ void nbp_hm_weight_kernel(NBP_HM_WEIGHT_ARGS);
__global__ void nbp_hm_draw_kernel(NBP_HM_DRAW_ARGS);
__global__ void nbp_hm_search_eval_kernel(NBP_HM_SEARCH_ARGS);
#endif
