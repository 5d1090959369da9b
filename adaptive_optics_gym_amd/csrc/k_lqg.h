// K25: the LQG controller (include/aogym_lqg.h).  Per (env, mode) a Kalman filter on S AR(2) sub-models, n = 2 S states: the steady-state
// gain from a fixed number of Riccati iterations (k_lqg_solve) and the three filter lines of a frame (k_lqg_update).  One thread per
// (env, mode); the records are [B][row][A] float64, mode innermost, so a wave reads and writes whole rows.  Every product, sum and
// quotient is one rounded float64 operation in the order the header writes out (mul_rn / add_rn, plain /): tests/lqg_reference.py replays
// the kernels bit for bit.  Every loop over the state is unrolled at compile time: P, K, c and xhat live in registers, never in scratch.
#pragma once
#include "k_common.h"

namespace aog {

// the rows of an env's record: a [S][2] | q [S] | r | K [n] | c_d [n] | convergence | solved | xhat [n] | command
__host__ __device__ constexpr int lqg_row_q(int S) { return 2 * S; }
__host__ __device__ constexpr int lqg_row_r(int S) { return 3 * S; }
__host__ __device__ constexpr int lqg_row_gain(int S) { return 3 * S + 1; }
__host__ __device__ constexpr int lqg_row_c(int S) { return 5 * S + 1; }
__host__ __device__ constexpr int lqg_row_conv(int S) { return 7 * S + 1; }
__host__ __device__ constexpr int lqg_row_solved(int S) { return 7 * S + 2; }
__host__ __device__ constexpr int lqg_row_x(int S) { return 7 * S + 3; }
__host__ __device__ constexpr int lqg_row_cmd(int S) { return 9 * S + 3; }
__host__ __device__ constexpr int lqg_rows(int S) { return 9 * S + 4; }

// (env, mode) of a flat thread index; false when it lies past the batch or the mask leaves the env out
__device__ __forceinline__ bool lqg_cell(const uint8_t* __restrict__ mask, int B, int A, int& b, int& j) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * A) return false;
  b = (int)(t / A);
  j = (int)(t - (long long)b * A);
  return !mask || mask[b];
}

__global__ __launch_bounds__(256) void k_lqg_set_model(double* __restrict__ rec, const double* __restrict__ a, const double* __restrict__ q,
                                                       const double* __restrict__ r, const uint8_t* __restrict__ mask, int B, int A, int S) {
  int b, j;
  if (!lqg_cell(mask, B, A, b, j)) return;
  double* p = rec + (size_t)b * lqg_rows(S) * A + j;
  for (int row = 0; row < 2 * S; ++row) p[(size_t)row * A] = a[((size_t)b * 2 * S + row) * A + j];
  for (int s = 0; s < S; ++s) p[(size_t)(lqg_row_q(S) + s) * A] = q[((size_t)b * S + s) * A + j];
  p[(size_t)lqg_row_r(S) * A] = r[(size_t)b * A + j];
  for (int row = lqg_row_gain(S); row < lqg_rows(S); ++row) p[(size_t)row * A] = 0.0;
}

__global__ __launch_bounds__(256) void k_lqg_reset(double* __restrict__ rec, const uint8_t* __restrict__ mask, int B, int A, int S) {
  int b, j;
  if (!lqg_cell(mask, B, A, b, j)) return;
  double* p = rec + (size_t)b * lqg_rows(S) * A + j;
  for (int row = lqg_row_x(S); row < lqg_rows(S); ++row) p[(size_t)row * A] = 0.0;
}

// 1 into *all when every (env, mode) is solved, 0 otherwise: one workgroup
__global__ __launch_bounds__(256) void k_lqg_all_solved(const double* __restrict__ rec, int* __restrict__ all, int B, int A, int S) {
  int ok = 1;
  for (long long t = threadIdx.x; t < (long long)B * A; t += blockDim.x) {
    const long long b = t / A;
    ok &= rec[((size_t)b * lqg_rows(S) + lqg_row_solved(S)) * A + (size_t)(t - b * A)] == 1.0;
  }
  ok = __syncthreads_and(ok);
  if (threadIdx.x == 0) *all = ok;
}

// pc = P C', s_ = C P C' + r, K = pc / s_ from the upper triangle of P
template <int S>
__device__ __forceinline__ void lqg_gain(const double (&P)[2 * S][2 * S], double r, double (&pc)[2 * S], double (&K)[2 * S]) {
  constexpr int N = 2 * S;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double acc = P[0][i];   // P(i, 0)
#pragma unroll
    for (int s = 1; s < S; ++s) acc = add_rn(acc, i <= 2 * s ? P[i][2 * s] : P[2 * s][i]);
    pc[i] = acc;
  }
  double sv = pc[0];
#pragma unroll
  for (int s = 1; s < S; ++s) sv = add_rn(sv, pc[2 * s]);
  sv = add_rn(sv, r);
#pragma unroll
  for (int i = 0; i < N; ++i) K[i] = pc[i] / sv;
}

template <int S>
__device__ __forceinline__ double lqg_trace(const double (&P)[2 * S][2 * S]) {
  double t = P[0][0];
#pragma unroll
  for (int i = 1; i < 2 * S; ++i) t = add_rn(t, P[i][i]);
  return t;
}

// P (entries i <= k only: 36 doubles at S = 4), a1, a2, q, pc and K are all the registers of a lane; the iteration loop is not unrolled
template <int S>
__global__ __launch_bounds__(256) void k_lqg_solve(double* __restrict__ rec, double* __restrict__ conv_out, const uint8_t* __restrict__ mask, int B,
                                                   int A, int delay, int iterations) {
  constexpr int N = 2 * S;
  int b, j;
  if (!lqg_cell(mask, B, A, b, j)) return;
  double* p = rec + (size_t)b * lqg_rows(S) * A + j;
  double a1[S], a2[S], q[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a1[s] = p[(size_t)(2 * s) * A];
    a2[s] = p[(size_t)(2 * s + 1) * A];
    q[s] = p[(size_t)(lqg_row_q(S) + s) * A];
  }
  const double r = p[(size_t)lqg_row_r(S) * A];
  double P[N][N], pc[N], K[N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = i; k < N; ++k) P[i][k] = (i == k && (i & 1) == 0) ? q[i >> 1] : 0.0;
  double t_last = lqg_trace<S>(P), t_prev = t_last;
#pragma unroll 1
  for (int it = 0; it < iterations; ++it) {
    lqg_gain<S>(P, r, pc, K);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int k = i; k < N; ++k) P[i][k] = add_rn(P[i][k], -mul_rn(K[i], pc[k]));   // M = P - K (C P), in place
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = s; t < S; ++t) {
        const double m00 = P[2 * s][2 * t], m01 = P[2 * s][2 * t + 1], m10 = s == t ? P[2 * s][2 * s + 1] : P[2 * s + 1][2 * t],
                     m11 = P[2 * s + 1][2 * t + 1];
        const double n00 = add_rn(mul_rn(a1[s], m00), mul_rn(a2[s], m10));
        const double n01 = add_rn(mul_rn(a1[s], m01), mul_rn(a2[s], m11));
        const double p00 = add_rn(mul_rn(n00, a1[t]), mul_rn(n01, a2[t]));
        P[2 * s][2 * t] = s == t ? add_rn(p00, q[s]) : p00;
        P[2 * s][2 * t + 1] = n00;
        if (s < t) P[2 * s + 1][2 * t] = add_rn(mul_rn(m00, a1[t]), mul_rn(m01, a2[t]));
        P[2 * s + 1][2 * t + 1] = m00;
      }
    t_prev = t_last;
    t_last = lqg_trace<S>(P);
  }
  lqg_gain<S>(P, r, pc, K);
  double c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = (i & 1) ? 0.0 : 1.0;
  for (int d = 0; d < delay; ++d)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double c0 = c[2 * s];
      c[2 * s] = add_rn(mul_rn(c0, a1[s]), c[2 * s + 1]);
      c[2 * s + 1] = mul_rn(c0, a2[s]);
    }
  double conv = __builtin_fabs(add_rn(t_last, -t_prev)) / t_last;
  bool usable = r > 0.0;   // and every sub-model stable: the roots of z^2 - a1 z - a2 inside the unit circle (a NaN fails every test)
#pragma unroll
  for (int s = 0; s < S; ++s) usable = usable && __builtin_fabs(a2[s]) < 1.0 && add_rn(a1[s], a2[s]) < 1.0 && add_rn(a2[s], -a1[s]) < 1.0;
  if (!usable) conv = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < N; ++i) {
    p[(size_t)(lqg_row_gain(S) + i) * A] = K[i];
    p[(size_t)(lqg_row_c(S) + i) * A] = c[i];
  }
  p[(size_t)lqg_row_conv(S) * A] = conv;
  p[(size_t)lqg_row_solved(S) * A] = 1.0;
  if (conv_out) conv_out[(size_t)b * A + j] = conv;
}

// A workgroup holds epb = 256 / A whole envs (thread = env el = tid / A of them, mode tid mod A): whether a row of y is finite is settled
// inside the workgroup, through one LDS word per env.  Grid: ceil(B / epb).
template <int S>
__global__ __launch_bounds__(256) void k_lqg_update(double* __restrict__ rec, const double* __restrict__ y, double* __restrict__ out,
                                                    const uint8_t* __restrict__ mask, int B, int A, int epb) {
  constexpr int N = 2 * S;
  __shared__ int bad[256];
  const int el = (int)threadIdx.x / A, j = (int)threadIdx.x - el * A;
  const long long bl = (long long)blockIdx.x * epb + el;
  const bool live = el < epb && bl < B;
  const int b = (int)bl;
  bad[threadIdx.x] = 0;
  __syncthreads();
  double yv = 0.0;
  if (live) {
    yv = y[(size_t)b * A + j];
    if (!__builtin_isfinite(yv)) bad[el] = 1;   // (every writer stores the same word)
  }
  __syncthreads();
  if (!live) return;
  double* p = rec + (size_t)b * lqg_rows(S) * A + j;
  if ((mask && !mask[b]) || bad[el]) {
    out[(size_t)b * A + j] = p[(size_t)lqg_row_cmd(S) * A];
    return;
  }
  double x[N];
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = p[(size_t)(lqg_row_x(S) + i) * A];
  double cx = x[0];
#pragma unroll
  for (int s = 1; s < S; ++s) cx = add_rn(cx, x[2 * s]);
  const double e = add_rn(yv, -cx);
  double u = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    x[i] = add_rn(x[i], mul_rn(p[(size_t)(lqg_row_gain(S) + i) * A], e));
    const double term = mul_rn(p[(size_t)(lqg_row_c(S) + i) * A], x[i]);
    u = i == 0 ? term : add_rn(u, term);
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    p[(size_t)(lqg_row_x(S) + 2 * s) * A] = add_rn(mul_rn(p[(size_t)(2 * s) * A], x[2 * s]), mul_rn(p[(size_t)(2 * s + 1) * A], x[2 * s + 1]));
    p[(size_t)(lqg_row_x(S) + 2 * s + 1) * A] = x[2 * s];
  }
  p[(size_t)lqg_row_cmd(S) * A] = u;
  out[(size_t)b * A + j] = u;
}

}  // namespace aog
