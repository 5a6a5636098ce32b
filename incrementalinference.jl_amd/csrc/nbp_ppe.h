// nbp_ppe.h -- point estimates of resident beliefs: calcPPE (services/FGOSUtils.jl:237-275), what setPPE! stores at the end of
// every setValKDE! (services/FactorGraph.jl:200-213).  DESIGN.md 3 holds the definition:
//   mean[d]   = mean(M, pts, GeodesicInterpolation()) of coordinate d over the points the belief holds (mean_geodesic_coord, the
//               function the proposals' spread statistics call, in the workgroup shape they call it in)
//   p_i       = sum_{j < c} exp(e(x_i, x_j)), e the exponent of nbp_kde.h over all D coordinates, the self term included, no
//               normalisation, j = 0 .. c - 1 in that order (one lane adds one p_i: reproducible bit for bit)
//   max_index = the smallest i whose p_i is the greatest (Julia's argmax); max = that point, copied
// A bandwidth entry that is not a positive finite number: max = NaN, max_index = -1; the mean is delivered all the same.
#pragma once
#include "nbp_kernels.h"
#include "nbp_kde.h"


// one record per belief; entries beyond the manifold's dimension are zero
struct nbp_ppe_rec {
  double mean[NBP_MAXD];
  double max[NBP_MAXD];
  int32_t max_index;
  int32_t pad;
};

#define NBP_PPE_ARGS const int32_t *slots, const int32_t *manifolds, const double *arena, int N, int64_t S, nbp_ppe_rec *out
#if NBP_TU & NBP_TU_PPE
// One workgroup per belief, 64 ceil(N / 64) lanes (the proposal kernels' shape: mean_geodesic_coord and block_sum see what they see
// there).  LDS: exp table | X[3][N] | red.  Lane i owns point i and walks j over the LDS rows (every lane of a wave reads the same
// address: broadcast reads); N^2 D operations per belief, no atomics, no pair symmetry.  The manifold is a runtime value.
__global__ void __launch_bounds__(512)
nbp_ppe_kernel(NBP_PPE_ARGS) {
  extern __shared__ double smem[];
  double *tab = smem, *X = smem + NBP_EXPTAB, *red = X + 3 * N;
  const double *s = arena + S * slots[blockIdx.x];
  const int M = manifolds[blockIdx.x], D = mani_dim(M), n = threadIdx.x;
  const int c = slot_count(s, N);
  nbp_exp_tab_init(tab);
  if (n < c)
    for (int k = 0; k < D; k++) X[k * N + n] = s[k * N + n];
  __syncthreads();
  // (three scalars: an array indexed by the loop lives in scratch)
  const double mu0 = mean_geodesic_coord(X, c, M, 0, red);
  const double mu1 = D > 1 ? mean_geodesic_coord(X + N, c, M, 1, red) : 0.0;
  const double mu2 = D > 2 ? mean_geodesic_coord(X + 2 * N, c, M, 2, red) : 0.0;
  const double h0 = s[3 * N], h1 = D > 1 ? s[3 * N + 1] : 1.0, h2 = D > 2 ? s[3 * N + 2] : 1.0;
  const bool valid = kde_bw_ok(h0) & kde_bw_ok(h1) & kde_bw_ok(h2);  // block-uniform
  double p = -INFINITY;
  int best = 0x7fffffff;
  if (valid && n < c) {
    const double r0 = 1.0 / h0, r1 = 1.0 / h1, r2 = 1.0 / h2;
    const bool c0 = is_circ(M, 0), c2 = is_circ(M, 2);
    const double x0 = X[n], x1 = D > 1 ? X[N + n] : 0.0, x2 = D > 2 ? X[2 * N + n] : 0.0;
    p = 0.0;
    best = n;
    for (int j = 0; j < c; j++) p += exp_nonpos(kde_exponent(x0, x1, x2, X, N, j, true, D > 1, D > 2, c0, c2, r0, r1, r2), tab);
  }
  // argmax on (value, index): the greater value, the lower index among equals -- inside the wave, then across the waves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double op = __shfl_xor(p, o, 64);
    const int ob = __shfl_xor(best, o, 64);
    if (op > p || (op == p && ob < best)) {
      p = op;
      best = ob;
    }
  }
  int *redi = (int *)(red + 32);
  __syncthreads();  // the reductions of the means are done with `red`
  if ((n & 63) == 0) {
    red[n >> 6] = p;
    redi[n >> 6] = best;
  }
  __syncthreads();
  if (n == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; w++)  // (the waves hold increasing indices: strictly greater keeps the lowest among equals)
      if (red[w] > p) {
        p = red[w];
        best = redi[w];
      }
    const bool found = valid && best >= 0 && best < c;
    const int bi = found ? best : 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    nbp_ppe_rec *r = out + blockIdx.x;
    r->mean[0] = mu0;
    r->mean[1] = mu1;
    r->mean[2] = mu2;
    r->max[0] = found ? X[bi] : nan;
    r->max[1] = D > 1 ? (found ? X[N + bi] : nan) : 0.0;
    r->max[2] = D > 2 ? (found ? X[2 * N + bi] : nan) : 0.0;
    r->max_index = found ? best : -1;
    r->pad = 0;
  }
}
#else
__global__ void nbp_ppe_kernel(NBP_PPE_ARGS);
#endif

static inline size_t nbp_ppe_lds_bytes(int N) { return ((size_t)NBP_EXPTAB + 3 * (size_t)N + NBP_RED) * 8; }
