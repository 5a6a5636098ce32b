// Prototype of the bandwidth fit's likelihood evaluation in single precision (the "bracketing" evaluations of the golden-section
// search): what one evaluation costs per ordered pair on gfx950 for several forms of the pair loop.  One workgroup of 256 lanes
// per fit, N = 200 points, lane i owns point i, EV evaluations in a row at different bandwidths, chip-filling launch.
// Second part (k_once): every unordered pair visited ONCE by a wave-wide DPP rotation (wave_ror:1, or row_ror:1 inside rows of
// 16 lanes) against the library's ordered broadcast loop, N = 200 and 256, four 256-lane workgroups per CU: shader cycles of
// the pair loop per wave (s_memtime) and the launch time.
//   hipcc --offload-arch=gfx950 -O3 lcv_f32_proto.hip -o lcv_f32_proto && ./lcv_f32_proto
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#define N 200
#define NP 208  // N rounded up to a multiple of 8, the padding at a distance that underflows

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// V0: broadcast reads (ds_read_b128: four partners per read), self term included, removed afterwards (s - 1)
// V1: the same with the self term masked per pair (v_cndmask)
// V2: packed arithmetic (v_pk_add_f32 / v_pk_mul_f32), self term included
// V3: rotation: lane i reads x[i + t] (x stored twice), no self term by construction
template <int V>
__global__ void __launch_bounds__(256) k_eval(const double *pts, float *out, int EV) {
  __shared__ __attribute__((aligned(16))) float xs[2 * NP];
  const int i = threadIdx.x;
  const double *x = pts + (size_t)blockIdx.x * N;
  float acc_out = 0.f;
  for (int ev = 0; ev < EV; ev++) {
    const double h = 0.2 + 0.01 * ev;
    const double sc = sqrt(1.4426950408889634 / (2.0 * h * h));
    __syncthreads();
    for (int j = i; j < 2 * NP; j += 256) {
      const int jj = j < NP ? j : j - NP;
      xs[j] = (jj < N) ? (float)(x[jj] * sc) : 1e18f;
    }
    __syncthreads();
    const float xi = (i < N) ? xs[i] : 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (V == 0) {
      const float4 *x4 = (const float4 *)xs;
#pragma unroll 2
      for (int g = 0; g < NP / 4; g++) {
        const float4 y = x4[g];
        const float d0 = xi - y.x, d1 = xi - y.y, d2 = xi - y.z, d3 = xi - y.w;
        s0 += exp2_fast(-d0 * d0);
        s1 += exp2_fast(-d1 * d1);
        s2 += exp2_fast(-d2 * d2);
        s3 += exp2_fast(-d3 * d3);
      }
      s0 -= 1.0f;
    } else if (V == 1) {
      const float4 *x4 = (const float4 *)xs;
#pragma unroll 2
      for (int g = 0; g < NP / 4; g++) {
        const float4 y = x4[g];
        const float d0 = xi - y.x, d1 = xi - y.y, d2 = xi - y.z, d3 = xi - y.w;
        const int j = 4 * g;
        s0 += (j == i) ? 0.f : exp2_fast(-d0 * d0);
        s1 += (j + 1 == i) ? 0.f : exp2_fast(-d1 * d1);
        s2 += (j + 2 == i) ? 0.f : exp2_fast(-d2 * d2);
        s3 += (j + 3 == i) ? 0.f : exp2_fast(-d3 * d3);
      }
    } else if (V == 2) {
      typedef float v2f __attribute__((ext_vector_type(2)));
      const float4 *x4 = (const float4 *)xs;
      v2f sa = {0.f, 0.f}, sb = {0.f, 0.f};
      const v2f xi2 = {xi, xi};
#pragma unroll 2
      for (int g = 0; g < NP / 4; g++) {
        const float4 y = x4[g];
        const v2f ya = {y.x, y.y}, yb = {y.z, y.w};
        const v2f da = xi2 - ya, db = xi2 - yb;
        const v2f qa = -da * da, qb = -db * db;
        v2f ea, eb;
        ea.x = exp2_fast(qa.x); ea.y = exp2_fast(qa.y);
        eb.x = exp2_fast(qb.x); eb.y = exp2_fast(qb.y);
        sa += ea;
        sb += eb;
      }
      s0 = sa.x - 1.0f; s1 = sa.y; s2 = sb.x; s3 = sb.y;
    } else if (V == 3) {
      if (i < N) {
        // x stored twice at stride N (not NP) for the rotation: rebuild a private view through the first copy + wrap
        for (int t = 1; t + 3 < N; t += 4) {
          int j0 = i + t, j1 = j0 + 1, j2 = j0 + 2, j3 = j0 + 3;
          j0 -= (j0 >= N) ? N : 0; j1 -= (j1 >= N) ? N : 0; j2 -= (j2 >= N) ? N : 0; j3 -= (j3 >= N) ? N : 0;
          const float d0 = xi - xs[j0], d1 = xi - xs[j1], d2 = xi - xs[j2], d3 = xi - xs[j3];
          s0 += exp2_fast(-d0 * d0);
          s1 += exp2_fast(-d1 * d1);
          s2 += exp2_fast(-d2 * d2);
          s3 += exp2_fast(-d3 * d3);
        }
        for (int t = 1 + ((N - 1) & ~3); t < N; t++) {
          int j0 = i + t;
          j0 -= (j0 >= N) ? N : 0;
          const float d0 = xi - xs[j0];
          s0 += exp2_fast(-d0 * d0);
        }
      }
    }
    const float s = (s0 + s1) + (s2 + s3);
    acc_out += __logf(fmaxf(s, 1e-30f));
  }
  if (i < N) out[(size_t)blockIdx.x * N + i] = acc_out;
}

template <int V>
static void run(const char *name, const double *dp, float *dout, int fits, int EV, std::vector<float> *res) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  k_eval<V><<<fits, 256>>>(dp, dout, 2);
  hipDeviceSynchronize();
  hipEventRecord(a);
  k_eval<V><<<fits, 256>>>(dp, dout, EV);
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms;
  hipEventElapsedTime(&ms, a, b);
  const double pairs = (double)fits * EV * N * (N - 1);  // ordered pairs
  res->resize((size_t)fits * N);
  hipMemcpy(res->data(), dout, res->size() * 4, hipMemcpyDeviceToHost);
  double cs = 0;
  for (size_t q = 0; q < res->size(); q++) cs += (*res)[q];
  printf("%-44s %8.3f ms  %7.3f ps per ordered pair  = %7.3f ps per symmetric pair   checksum %.6e\n", name, ms, ms * 1e9 / pairs, 2 * ms * 1e9 / pairs, cs);
}

// ------------------------------------------------------------------------------------------------
// Pair-once schedule against the ordered loop.  M: 0 = ordered broadcast loop with the self term masked in the own wave's
// groups (the library's loop); 1 = wave_ror:1 rotation; 2 = row_ror:1 inside rows of 16 lanes, one cross-row step per 16
// (the partner's coordinate and sum move to the next row through ds_bpermute).  NN points; the waves of the W = NN / 64 full
// chunks run a diagonal block (t = 1 .. 32), floor((W - 1) / 2) whole blocks (t = 0 .. 63) and, for even W, half of the block
// opposite; the partial chunk's points arrive as broadcast partners, the partial wave sums over all partners.
#define ROR1(v) __builtin_amdgcn_mov_dpp((v), 0x13C, 0xF, 0xF, false)  // (every lane reads a lane: no old value to keep)
#define RROR1(v) __builtin_amdgcn_mov_dpp((v), 0x121, 0xF, 0xF, false)
__device__ __forceinline__ float ror_f(float v) { return __int_as_float(ROR1(__float_as_int(v))); }
__device__ __forceinline__ float rror_f(float v) { return __int_as_float(RROR1(__float_as_int(v))); }
// the rotating sum: with an old value of zero the compiler folds the rotation into the addition (v_add_f32_dpp)
__device__ __forceinline__ float ror_s(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x13C, 0xF, 0xF, false)); }
__device__ __forceinline__ float rror_s(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, false)); }
__device__ __forceinline__ float pair_e(float xi, float y) {
  const float d = xi - y;
  return exp2_fast(-d * d);
}
// n steps of one block by wave_ror: the first step without (first = false) or with a rotation; returns the partner sums,
// which sit first + n - 1 lanes from home
__device__ __forceinline__ float block_wave(float xi, float y, int n, bool first, float &o0, float &o1, float &o2, float &o3) {
  if (first) y = ror_f(y);
  float e = pair_e(xi, y), ps = e;
  o3 += e;
  int s = 1;
  for (; s + 3 < n; s += 4) {
    y = ror_f(y); e = pair_e(xi, y); o0 += e; ps = ror_s(ps) + e;
    y = ror_f(y); e = pair_e(xi, y); o1 += e; ps = ror_s(ps) + e;
    y = ror_f(y); e = pair_e(xi, y); o2 += e; ps = ror_s(ps) + e;
    y = ror_f(y); e = pair_e(xi, y); o3 += e; ps = ror_s(ps) + e;
  }
  for (; s < n; s++) {
    y = ror_f(y); e = pair_e(xi, y); o0 += e; ps = ror_s(ps) + e;
  }
  return ps;
}
// the same by row_ror (a timing stand-in: the full blocks visit the right pairs, the diagonal and half blocks the right NUMBER
// of pairs, so its checksum differs): lane l of row r meets (row r - R, lane l - t) for R = 0 .. n / 16 - 1, t = 0 .. 15 (first: from t = 1,
// R = 0 on: n steps); moving on by a row is one ds_bpermute of the coordinate and of the sum
__device__ __forceinline__ float block_row(float xi, float y, int n, bool first, int lane, float &o0, float &o1, float &o2, float &o3) {
  const int up = ((((lane >> 4) - 1) & 3) * 16 + ((lane - 1) & 15)) << 2;  // from (row - 1, column - 1): the sixteenth column step and the row step in one
  float ps = 0.f;
  int s = first ? 1 : 0;
  const int end = s + n;
  if (first) y = rror_f(y);
  while (s < end) {
    const int m = min(end, (s & ~15) + 16);
    for (; s < m; s++) {
      const float e = pair_e(xi, y);
      o0 += e;
      ps += e;
      if (s + 1 < m) { y = rror_f(y); ps = rror_s(ps); }
    }
    if (s < end) {
      y = __int_as_float(__builtin_amdgcn_ds_bpermute(up, __float_as_int(y)));
      ps = __int_as_float(__builtin_amdgcn_ds_bpermute(up, __float_as_int(ps)));
    }
  }
  return ps;
}
template <int M, int NN>
__global__ void __launch_bounds__(256) k_once(const double *pts, float *out, int EV, unsigned long long *cyc) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // (sized by the host so that four workgroups share a CU)
  constexpr int W = NN >> 6, G4 = (NN + 3) >> 2, KF = (W - 1) / 2, ROWS = 1 + KF + ((W & 1) ? 0 : 1);
  float *xs = sm, *rows = sm + 4 * G4;
  const int i = threadIdx.x, l = i & 63, w = __builtin_amdgcn_readfirstlane(i >> 6);
  const double *x = pts + (size_t)blockIdx.x * NN;
  for (int j = i; j < ROWS * 64 * W; j += 256) rows[j] = 0.f;
  float acc_out = 0.f;
  unsigned long long cy = 0;
  for (int ev = 0; ev < EV; ev++) {
    const double h = 0.2 + 0.01 * ev;
    const double sc = sqrt(1.4426950408889634 / (2.0 * h * h));
    __syncthreads();
    for (int j = i; j < 4 * G4; j += 256) xs[j] = (j < NN) ? (float)(x[j] * sc) : 0.f;
    __syncthreads();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    const float xi = (i < NN) ? xs[i] : 0.f;
    const float4 *x4 = (const float4 *)xs;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    auto ordered = [&](int ga, int gb, bool mask) {
#pragma unroll 2
      for (int g = ga; g < gb; g++) {
        const float4 y = x4[g];
        float e0 = pair_e(xi, y.x), e1 = pair_e(xi, y.y), e2 = pair_e(xi, y.z), e3 = pair_e(xi, y.w);
        const int j = 4 * g;
        if (mask) {
          e0 = (j == i || j >= NN) ? 0.f : e0;
          e1 = (j + 1 == i || j + 1 >= NN) ? 0.f : e1;
          e2 = (j + 2 == i || j + 2 >= NN) ? 0.f : e2;
          e3 = (j + 3 == i || j + 3 >= NN) ? 0.f : e3;
        }
        s0 += e0; s1 += e1; s2 += e2; s3 += e3;
      }
    };
    if (M == 0 || w >= W) {
      if (i < NN) {
        const int o0 = w * 16;
        ordered(0, min(o0, NN >> 2), false);
        ordered(min(o0, NN >> 2), min(o0 + 16, NN >> 2), true);
        ordered(min(o0 + 16, NN >> 2), NN >> 2, false);
        if (NN & 3) ordered(NN >> 2, G4, true);
      }
    } else {
      auto put = [&](int r, int chunk, int off, float ps) { rows[(r * W + chunk) * 64 + ((l - off) & 63)] = ps; };
      float ps;
      // diagonal: t = 1 .. 31 to both ends, t = 32 to the own sum only (the lane 32 away does the same for its end)
      if (M == 1) {
        ps = block_wave(xi, xi, 31, true, s0, s1, s2, s3);
        s0 += pair_e(xi, __shfl(xi, l ^ 32, 64));
      } else {
        ps = block_row(xi, xi, 31, true, l, s0, s1, s2, s3);
        s0 += pair_e(xi, __shfl(xi, l ^ 32, 64));
      }
      put(0, w, 31, ps);
      for (int k = 1; k <= KF; k++) {
        int c = w + k;
        c -= (c >= W) ? W : 0;
        const float y = xs[64 * c + l];
        ps = (M == 1) ? block_wave(xi, y, 64, false, s0, s1, s2, s3) : block_row(xi, y, 64, false, l, s0, s1, s2, s3);
        put(k, c, 63, ps);
      }
      if ((W & 1) == 0) {
        const bool hi = w >= W / 2;
        const int c = hi ? w - W / 2 : w + W / 2;
        const float y = xs[64 * c + l];
        ps = (M == 1) ? block_wave(xi, y, 32, hi, s0, s1, s2, s3) : block_row(xi, y, 32, hi, l, s0, s1, s2, s3);
        put(KF + 1, c, hi ? 32 : 31, ps);
      }
      ordered(16 * W, NN >> 2, false);
      if (NN & 3) ordered(NN >> 2, G4, true);
    }
    float s = (s0 + s1) + (s2 + s3);
    cy += __builtin_amdgcn_s_memtime() - c0;
    __syncthreads();
    if (M != 0 && i < 64 * W) {
      for (int r = 0; r < ROWS; r++) {
        s += rows[r * 64 * W + i];
        rows[r * 64 * W + i] = 0.f;
      }
    }
    acc_out += __logf(fmaxf(s, 1e-30f));
  }
  if (i < NN) out[(size_t)blockIdx.x * NN + i] = acc_out;
  if (l == 0 && w < W) atomicAdd(cyc, cy);
}

template <int M, int NN>
static void run_once(const char *name, const double *dp, float *dout, int fits, int EV, unsigned long long *dcyc) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  const size_t lds = 36 * 1024;  // 160 KB per CU: four workgroups
  k_once<M, NN><<<fits, 256, lds>>>(dp, dout, 2, dcyc);
  hipDeviceSynchronize();
  hipMemset(dcyc, 0, 8);
  hipEventRecord(a);
  k_once<M, NN><<<fits, 256, lds>>>(dp, dout, EV, dcyc);
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms;
  hipEventElapsedTime(&ms, a, b);
  unsigned long long cy = 0;
  hipMemcpy(&cy, dcyc, 8, hipMemcpyDeviceToHost);
  std::vector<float> r((size_t)fits * NN);
  hipMemcpy(r.data(), dout, r.size() * 4, hipMemcpyDeviceToHost);
  double cs = 0;
  for (float v : r) cs += v;
  constexpr int W = NN >> 6;
  // unordered pairs a full wave's lane covers per evaluation: (NN - 1) / 2 among full chunks on average, counted as the
  // ordered loop's NN - 1 partners halved, so that both forms divide by the same number
  const double wave_evals = (double)fits * EV * W, upairs = 0.5 * (NN - 1);
  printf("N %d %-34s %8.3f ms  %8.0f cycles per wave and evaluation (four waves a SIMD)  %6.2f cycles per unordered pair and wave, /4 = %5.2f per SIMD   checksum %.6e\n",
         NN, name, ms, cy / wave_evals, cy / wave_evals / upairs, cy / wave_evals / upairs / 4, cs);
}

int main(int argc, char **argv) {
  const int fits = argc > 1 ? atoi(argv[1]) : 8192, EV = argc > 2 ? atoi(argv[2]) : 16;
  std::vector<double> p((size_t)fits * N);
  srand(1);
  for (auto &v : p) {
    double u1 = (rand() + 1.0) / (RAND_MAX + 2.0), u2 = (rand() + 1.0) / (RAND_MAX + 2.0);
    v = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2);
  }
  double *dp;
  float *dout;
  hipMalloc(&dp, p.size() * 8);
  hipMalloc(&dout, p.size() * 4);
  hipMemcpy(dp, p.data(), p.size() * 8, hipMemcpyHostToDevice);
  std::vector<float> r;
  printf("fits %d, N %d, %d evaluations each (the double-precision loop of the library: 0.765 ps per symmetric pair)\n", fits, N, EV);
  run<0>("V0 broadcast b128, self term subtracted", dp, dout, fits, EV, &r);
  run<1>("V1 broadcast b128, self term masked", dp, dout, fits, EV, &r);
  run<2>("V2 packed f32, self term subtracted", dp, dout, fits, EV, &r);
  run<3>("V3 rotation (per-lane reads)", dp, dout, fits, EV, &r);
  {  // pair-once schedule: the first `fits * 200` doubles serve as `fits * 200 / NN` clouds of NN points
    unsigned long long *dcyc;
    hipMalloc(&dcyc, 8);
    const int f2 = fits * N / 256;
    run_once<0, 200>("ordered broadcast, masked", dp, dout, f2, EV, dcyc);
    run_once<1, 200>("pair once, wave_ror:1", dp, dout, f2, EV, dcyc);
    run_once<2, 200>("pair once, row_ror:1 + bpermute", dp, dout, f2, EV, dcyc);
    run_once<0, 256>("ordered broadcast, masked", dp, dout, f2, EV, dcyc);
    run_once<1, 256>("pair once, wave_ror:1", dp, dout, f2, EV, dcyc);
    run_once<2, 256>("pair once, row_ror:1 + bpermute", dp, dout, f2, EV, dcyc);
  }
  return 0;
}
