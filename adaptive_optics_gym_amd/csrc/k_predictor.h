// K17: the recursive-least-squares predictor of aog_predictor_update, one workgroup per env, everything float64 without fused multiply-add.
//
// Per env the handle keeps ONE record of (n A + n^2 + n + 2) 8-byte words, n = A order: W [n][A], P [n][n], the history [n] (newest
// measurement first, already divided by scale), then count and skipped as int64.  The records of a handle lie one behind the other: that
// array is the state blob of aog_predictor_get_state as it stands.
//
// Work split of a workgroup of NW waves: wave w owns the rows [w rpw, (w + 1) rpw) of P and of W, lane l the columns l, l + 64, ...  Every
// product against a vector (g = P x, W' x) is a column sum: lane l adds its rows in ascending order, the NW partial sums of a column go
// through the LDS and one thread adds them in wave order.  (P is symmetric bit for bit — g_i g_j is formed before anything else touches it
// — so the column sums of P are P x.)  x' g is summed by every wave alike: lane l adds i = l, l + 64, ... ascending, then a 6-step
// butterfly over the lanes, whose result is the same bits in every lane because a + b = b + a.  None of these orders depends on the batch
// or on where the env sits in it: a split batch reproduces the whole one bit for bit.
//
// Traffic per env and update.  Register form (n <= 128): the wave's block of P and of W is loaded once into registers (at most 32 + 32
// float64 per lane), updated there and stored once: 8 n^2 + 8 n A bytes read, as many written = 16 n^2 + 16 n A.  Two-read form (n from
// 129 to 256, where a workgroup's registers no longer hold the 512 KB of P): P and W are read for the sums, read again for the update and
// written once = 24 n^2 + 24 n A bytes; the second read comes out of the caches where they still hold it.  Plain stores only (vector
// stores), no atomics, no float32 anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aog {

constexpr int kPredMaxN = 256;   // n = act_dim * order, and act_dim alone
constexpr int kPredKeepN = 128;  // largest n of the register form

struct PredictorArgs {
  char* state;           // [B] records
  size_t rec_bytes;
  const double* y;       // [B][A]
  const uint8_t* mask;   // nullable [B]
  double* pred;          // [B][A]
  double* innov;         // nullable [B][A]
  int A, order, n;
  double lam, scale, p0;
};

__host__ __device__ inline size_t predictor_record_words(int A, int n) { return (size_t)n * A + (size_t)n * n + n + 2; }
// float64 words of dynamic LDS: x_old [n], x_new [n], g [n], k = g / d [n], e [A], y [A], partial sums [NW][n] and [NW][A]
__host__ __device__ inline size_t predictor_lds_words(int A, int n, int nw) { return (size_t)4 * n + 2 * A + (size_t)nw * (n + A); }

__device__ inline bool pred_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }

template <int NW, int RPW, int CB, int CBW, bool KEEP>
__global__ __launch_bounds__(NW * 64) void k_predictor_update(PredictorArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x;
  if (a.mask && !a.mask[b]) return;
  extern __shared__ double lds_pred[];
  const int n = a.n, A = a.A, t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* xo = lds_pred;
  double* xn = xo + n;
  double* gs = xn + n;
  double* ks = gs + n;
  double* es = ks + n;
  double* ys = es + A;
  double* pg = ys + A;
  double* pw = pg + (size_t)NW * n;
  double* W = reinterpret_cast<double*>(a.state + (size_t)b * a.rec_bytes);
  double* P = W + (size_t)n * A;
  double* H = P + (size_t)n * n;
  long long* cs = reinterpret_cast<long long*>(H + n);
  const size_t row_b = (size_t)b * A;

  int bad = 0;
  if (t < A) {
    const double v = a.y[row_b + t];
    ys[t] = v;
    bad = !pred_finite(v);
  }
  if (t < n) xo[t] = H[t];
  const long long cnt = cs[0];
  bad = __syncthreads_or(bad);
  if (bad) {   // a non-finite measurement: the state stays, the prediction is the measurement
    if (t < A) {
      a.pred[row_b + t] = ys[t];
      if (a.innov) a.innov[row_b + t] = 0.0;
    }
    if (t == 0) cs[1] = cs[1] + 1;
    return;
  }
  if (t < n) xn[t] = t < A ? ys[t] / a.scale : xo[t - A];
  const bool have = cnt >= (long long)a.order;   // a previous regressor exists (uniform over the workgroup)
  if (!have) {
    if (t < A) {
      a.pred[row_b + t] = ys[t];
      if (a.innov) a.innov[row_b + t] = 0.0;
    }
    __syncthreads();
    if (t < n) H[t] = xn[t];
    if (t == 0) cs[0] = cnt + 1;
    return;
  }

  constexpr int UR = KEEP ? RPW : 4;   // the register form unrolls its rows in full: its arrays must stay in registers
  const int rpw = KEEP ? RPW : (n + NW - 1) / NW;
  const int row0 = w * rpw;
  double pr[KEEP ? RPW * CB : 1], wr[KEEP ? RPW * CBW : 1];
  if constexpr (KEEP) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int row = row0 + r;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int col = lane + 64 * cb;
        pr[r * CB + cb] = (row < n && col < n) ? P[(size_t)row * n + col] : 0.0;
      }
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) {
        const int col = lane + 64 * cb;
        wr[r * CBW + cb] = (row < n && col < A) ? W[(size_t)row * A + col] : 0.0;
      }
    }
  }
  __syncthreads();   // xo, xn

  // column sums over the wave's rows: g = P x_old and W' x_old
  {
    double ag[CB], aw[CBW];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) ag[cb] = 0.0;
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) aw[cb] = 0.0;
#pragma unroll UR
    for (int r = 0; r < rpw; ++r) {
      const int row = row0 + r;
      if (row < n) {
        const double xr = xo[row];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const int col = lane + 64 * cb;
          double v;
          if constexpr (KEEP) v = pr[r * CB + cb];
          else v = col < n ? P[(size_t)row * n + col] : 0.0;
          ag[cb] = ag[cb] + v * xr;
        }
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          const int col = lane + 64 * cb;
          double v;
          if constexpr (KEEP) v = wr[r * CBW + cb];
          else v = col < A ? W[(size_t)row * A + col] : 0.0;
          aw[cb] = aw[cb] + v * xr;
        }
      }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int col = lane + 64 * cb;
      if (col < n) pg[(size_t)w * n + col] = ag[cb];
    }
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) {
      const int col = lane + 64 * cb;
      if (col < A) pw[(size_t)w * A + col] = aw[cb];
    }
  }
  __syncthreads();
  double e = 0.0;
  if (t < n) {
    double g = pg[t];
    for (int k = 1; k < NW; ++k) g = g + pg[(size_t)k * n + t];
    gs[t] = g;
  }
  if (t < A) {
    double s = pw[t];
    for (int k = 1; k < NW; ++k) s = s + pw[(size_t)k * A + t];
    e = xn[t] - s;
    es[t] = e;
  }
  __syncthreads();
  double d;
  {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s = s + xo[i] * gs[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    d = a.lam + s;
  }
  if (t < n) ks[t] = gs[t] / d;
  __syncthreads();

  // the update, and the column sums W_new' x_new of the prediction
  {
    const bool scale_p = a.lam != 1.0;   // (v / 1 is v: the division is skipped, not changed)
    double gc[CB], ec[CBW], aw[CBW];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) gc[cb] = (lane + 64 * cb) < n ? gs[lane + 64 * cb] : 0.0;
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) {
      ec[cb] = (lane + 64 * cb) < A ? es[lane + 64 * cb] : 0.0;
      aw[cb] = 0.0;
    }
#pragma unroll UR
    for (int r = 0; r < rpw; ++r) {
      const int row = row0 + r;
      if (row < n) {
        const double gr = gs[row], kr = ks[row], xr = xn[row];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const int col = lane + 64 * cb;
          if (col < n) {
            double v;
            if constexpr (KEEP) v = pr[r * CB + cb];
            else v = P[(size_t)row * n + col];
            v = v - (gr * gc[cb]) / d;
            if (scale_p) v = v / a.lam;
            P[(size_t)row * n + col] = v;
          }
        }
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          const int col = lane + 64 * cb;
          if (col < A) {
            double v;
            if constexpr (KEEP) v = wr[r * CBW + cb];
            else v = W[(size_t)row * A + col];
            v = v + kr * ec[cb];
            W[(size_t)row * A + col] = v;
            aw[cb] = aw[cb] + v * xr;
          }
        }
      }
    }
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) {
      const int col = lane + 64 * cb;
      if (col < A) pw[(size_t)w * A + col] = aw[cb];   // (its last readers passed two barriers ago)
    }
  }
  __syncthreads();
  if (t < n) H[t] = xn[t];
  if (t == 0) cs[0] = cnt + 1;
  if (t < A) {
    double s = pw[t];
    for (int k = 1; k < NW; ++k) s = s + pw[(size_t)k * A + t];
    a.pred[row_b + t] = a.scale * s;
    if (a.innov) a.innov[row_b + t] = a.scale * e;
  }
}

// the state after create: W the persistence predictor, P = p0 I, an empty history, both counters 0
__global__ __launch_bounds__(256) void k_predictor_reset(PredictorArgs a) {
  const int b = blockIdx.x;
  if (a.mask && !a.mask[b]) return;
  const int n = a.n, A = a.A;
  double* W = reinterpret_cast<double*>(a.state + (size_t)b * a.rec_bytes);
  double* P = W + (size_t)n * A;
  double* H = P + (size_t)n * n;
  long long* cs = reinterpret_cast<long long*>(H + n);
  for (int i = threadIdx.x; i < n * A; i += 256) W[i] = (i / A == i % A) ? 1.0 : 0.0;
  for (int i = threadIdx.x; i < n * n; i += 256) P[i] = (i / n == i % n) ? a.p0 : 0.0;
  for (int i = threadIdx.x; i < n; i += 256) H[i] = 0.0;
  if (threadIdx.x < 2) cs[threadIdx.x] = 0;
}

}  // namespace aog
