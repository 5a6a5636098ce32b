// nbp_kde.h -- the arithmetic of a belief's kernel density estimate, stated once for every query on resident beliefs (nbp_ppe.h,
// nbp_query.h, nbp_stats.h, nbp_marginal.h).  DESIGN.md 3 holds the definition; coordinates are tangent coordinates at the identity
// (Euclid(1-3); the circle; SE(2): x, y, theta), K the set of coordinates that enter (all D of the manifold but for a marginal).
//   exponent  e(x, y_j) = -1/2 sum_{d in K} (delta_d(x, y_j) r_d)^2, r_d = 1 / h_d formed once by the caller, delta_d = x_d - y_jd,
//             wrapped to [-pi, pi) on circular coordinates BEFORE the multiplication by r_d; the squares are added in ascending
//             coordinate order, one rounding per written operation.
//   validity  a bandwidth entry takes part only if it is a positive finite number (what a caller delivers otherwise is its own rule).
//   norm      c prod_{d in K} sqrt(2 pi) h_d, the factors applied to (double)c in ascending coordinate order.
// The bit equalities the queries promise one another (the full-mask marginal and nbp_run_evaluate, the density at a belief's own
// points and the PPE's p_i, the logarithm of nbp_stats.h) hold because all of them call these functions.
#pragma once
#include "nbp_device.h"

#define NBP_SQRT_2PI 2.5066282746310002  // sqrt(2 pi), rounded to nearest

// e(x, y_j) for row j of Y[3][N].  k0, k1, k2: the coordinates that enter (block-uniform); c0, c2: coordinate 0 / 2 is circular
// (coordinate 1 never is).  (0 + d d = d d exactly: whichever coordinate enters first, it enters as if it had been assigned.)
__device__ __forceinline__ double kde_exponent(double x0, double x1, double x2, const double *Y, int N, int j, bool k0, bool k1, bool k2,
                                               bool c0, bool c2, double r0, double r1, double r2) {
  double e = 0.0;
  if (k0) {
    double d0 = x0 - Y[j];
    if (c0) d0 = wrap_pi(d0);
    d0 *= r0;
    e = d0 * d0;
  }
  if (k1) {
    const double d1 = (x1 - Y[N + j]) * r1;
    e += d1 * d1;
  }
  if (k2) {
    double d2 = x2 - Y[2 * N + j];
    if (c2) d2 = wrap_pi(d2);
    d2 *= r2;
    e += d2 * d2;
  }
  return -0.5 * e;
}

// (callers join the tests of several entries with `&`: block-uniform values, nothing to skip -- `&&` across the calls costs a branch each)
__device__ __forceinline__ bool kde_bw_ok(double h) { return h > 0.0 && h < INFINITY; }

__device__ __forceinline__ double kde_norm(int c, bool k0, bool k1, bool k2, double h0, double h1, double h2) {
  double norm = (double)c;
  if (k0) norm *= NBP_SQRT_2PI * h0;
  if (k1) norm *= NBP_SQRT_2PI * h1;
  if (k2) norm *= NBP_SQRT_2PI * h2;
  return norm;
}
