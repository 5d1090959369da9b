// K18: closed-loop modal telemetry (aog_telemetry_*): a ring of measurements per env, Welch's power spectral density of every mode over
// what the ring holds, and the integrator gain per mode that minimises the residual that density predicts.  Everything float64 without
// fused multiply-add, plain vector stores, no atomics.
//
// Per env the handle keeps ONE record of T A + 2 8-byte words: hist [T][A] float64 (sample number c in row c mod T), then count and
// skipped as int64.  The records of a handle lie one behind the other: that array is the state blob of aog_telemetry_get_state.
//
// k_telemetry_psd<S> — the transform is a float64 radix-2 FFT along time, in the LDS (profiles/telemetry.md says why not the dense DFT on
// the matrix cores).  A workgroup of 256 threads owns one env and M = min(64, 8192 / S) neighbouring modes; thread (js, m) = (t / M,
// t mod M) owns mode m and the rows r = js, js + P, ... (P = 256 / M) of every half segment, so at M = 64 a wave's load is one whole
// 512-byte piece of a row.  Segments overlap by half: the workgroup walks the nseg + 1 half segments oldest first, each thread keeps
// its rows of the previous half in registers, and so every row of the ring is read exactly once.  The ring's seam is resolved per half
// segment from one workgroup-uniform number (the rows left before row T).  Per segment:
//   mean     thread (js, m) adds its 2 E rows in ascending order, the P partial sums of a mode are added in js order, / S
//   window   (y - mean) w_n, w_n = (1 - cos(2 pi n / S)) / 2, into the LDS as z_n = y'_2n + i y'_2n+1     (n < S / 2)
//   FFT      length S / 2, decimation in frequency, in place, one barrier per stage; Z_k lands at the bit-reversed index
//   unpack   X_k = E_k + W_S^k O_k with E_k = (Z_k + conj Z_{S/2-k}) / 2, O_k = -i (Z_k - conj Z_{S/2-k}) / 2      (k = 0 .. S / 2)
//   sum      thread (js, m) owns the bins k = js, js + P, ...: acc_k += re^2 + im^2, in registers, segments oldest first
// and at the end Phi[k] = m_k (acc_k / nseg) / (S sum w^2), where S sum w^2 = 3 S^2 / 8 exactly for the periodic Hann window.  Phi goes
// through the LDS once more so that the rows of psd [B][A][S/2+1] are written along k.  The tail is aog_telemetry_gains':
// J(g) = sum_k |R_k(g)|^2 Phi[k], k = 1 .. S / 2 ascending, thread (js, m) the candidates g = js, js + P, ...; the first minimiser in
// grid order wins.  |R_k(g)|^2 depends on (k, g) alone: k_telemetry_rk builds it once per call ON THE DEVICE, float64.
// The cos / sin of the transform are sincospi of exact binary fractions, computed by every workgroup into its LDS (1.5 S values).
// No order of any sum depends on the batch, the mask or where the env sits: a split batch reproduces the whole one bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aog {

constexpr int kTelMaxA = 128;      // modes
constexpr int kTelMinT = 64, kTelMaxT = 1024, kTelMinS = 32;
constexpr int kTelMaxG = 64;       // gain candidates
constexpr int kTelMaxDelay = 4;
constexpr int kTelThreads = 256;

struct TelemetryArgs {
  char* state;           // [B] records
  size_t rec_bytes;
  const uint8_t* mask;   // nullable [B]
  int A, T;
  const double* y;       // push: [B][A]
  double* psd;           // nullable [B][A][S/2+1]
  int* segments;         // nullable [B]
  const double* r2;      // nullable: [G][S/2] |R_k(g)|^2 for k = 1 .. S/2, then the grid [G]   (k_telemetry_rk)
  double* gain;          // [B][A]      (with r2)
  double* cost;          // [B][A]
  double* cost_all;      // nullable [B][A][G]
  int G;
};

struct TelemetryRkArgs {
  double* r2;            // [G][S/2], then grid [G]
  int S, G, delay;
  double grid[kTelMaxG];
};

__host__ __device__ inline size_t telemetry_record_words(int A, int T) { return (size_t)T * A + 2; }

template <int S>
struct TelGeom {
  static constexpr int M = S <= 128 ? 64 : 8192 / S;   // modes of a workgroup
  static constexpr int P = kTelThreads / M;            // threads along time
  static constexpr int E = (S / 2) / P;                // rows of a half segment per thread
  static constexpr int N = S / 2;                      // length of the complex transform
  static constexpr int BF = (N / 2) / P;               // butterflies of a stage per thread
  static constexpr int NK = (S / 2 + P) / P;           // bins per thread: ceil((S / 2 + 1) / P)
  static constexpr int LOGN = S == 32 ? 4 : S == 64 ? 5 : S == 128 ? 6 : S == 256 ? 7 : S == 512 ? 8 : 9;
  // float64 words of dynamic LDS: the transform S M (later Phi [S/2+1][M+1]), the twiddles S, the partial sums P M, the candidates P M / 2
  static constexpr size_t kLdsWords = (size_t)S * M + S + kTelThreads + kTelThreads / 2;
  static_assert((S / 2 + 1) * (M + 1) <= S * M && E >= 1 && BF >= 1, "telemetry geometry");
};

__device__ inline bool tel_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }

// one row per selected env into the ring; a row with a non-finite value is counted in `skipped` instead
__global__ __launch_bounds__(kTelMaxA) void k_telemetry_push(TelemetryArgs a) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (a.mask && !a.mask[b]) return;
  double* hist = reinterpret_cast<double*>(a.state + (size_t)b * a.rec_bytes);
  long long* cs = reinterpret_cast<long long*>(hist + (size_t)a.T * a.A);
  double v = 0.0;
  if (t < a.A) v = a.y[(size_t)b * a.A + t];
  const long long cnt = cs[0];
  const int bad = __syncthreads_or(!tel_finite(v));
  if (bad) {
    if (t == 0) cs[1] = cs[1] + 1;
    return;
  }
  const int row = (int)(cnt & (long long)(a.T - 1));
  if (t < a.A) hist[(size_t)row * a.A + t] = v;
  if (t == 0) cs[0] = cnt + 1;
}

// the state after create: an empty ring of zeros, both counters 0
__global__ __launch_bounds__(256) void k_telemetry_reset(TelemetryArgs a) {
  const int b = blockIdx.x;
  if (a.mask && !a.mask[b]) return;
  double* hist = reinterpret_cast<double*>(a.state + (size_t)b * a.rec_bytes);
  long long* cs = reinterpret_cast<long long*>(hist + (size_t)a.T * a.A);
  for (int i = threadIdx.x; i < a.T * a.A; i += 256) hist[i] = 0.0;
  if (threadIdx.x < 2) cs[threadIdx.x] = 0;
}

// |R_k(g)|^2 = |1 - z^-1|^2 / |1 - z^-1 + g z^-d|^2 at z = exp(2 pi i k / S), one thread per (k, g), k = 1 .. S / 2; 1 - cos is formed as
// 2 sin^2 of the half angle.  Block y = the candidate; the grid itself is stored behind the table for the argmin's read.
__global__ __launch_bounds__(256) void k_telemetry_rk(TelemetryRkArgs a) {
#pragma clang fp contract(off)
  const int g = blockIdx.y, half = a.S / 2;
  const int k = 1 + (int)(blockIdx.x * 256 + threadIdx.x);
  const double gv = a.grid[g];
  if (k == 1) a.r2[(size_t)a.G * half + g] = gv;
  if (k > half) return;
  double sh, ch, s1, c1, sd, cd;
  sincospi((double)k / (double)a.S, &sh, &ch);
  sincospi(2.0 * (double)k / (double)a.S, &s1, &c1);
  const int kd = (k * a.delay) & (a.S - 1);
  sincospi(2.0 * (double)kd / (double)a.S, &sd, &cd);
  const double om = 2.0 * (sh * sh);   // 1 - cos
  const double re = om + gv * cd, im = s1 - gv * sd;
  a.r2[(size_t)g * half + (k - 1)] = (2.0 * om) / (re * re + im * im);
}

template <int S>
__global__ __launch_bounds__(kTelThreads) void k_telemetry_psd(TelemetryArgs a) {
#pragma clang fp contract(off)
  using Geo = TelGeom<S>;
  constexpr int M = Geo::M, P = Geo::P, E = Geo::E, N = Geo::N, BF = Geo::BF, NK = Geo::NK, H = S / 2, NB = S / 2 + 1;
  const int nmb = (a.A + M - 1) / M;
  const int b = blockIdx.x / nmb, mb = blockIdx.x - b * nmb;
  if (a.mask && !a.mask[b]) return;   // (workgroup-uniform, before any load)
  extern __shared__ __attribute__((aligned(16))) double lds_tel[];
  double2* work = reinterpret_cast<double2*>(lds_tel);   // [N][M]
  double* workd = lds_tel;
  double2* tw = reinterpret_cast<double2*>(lds_tel + (size_t)S * M);   // [S/2]: W_S^q = (cos, -sin)(2 pi q / S)
  double* part = lds_tel + (size_t)S * M + S;                          // [P][M]
  int* cand = reinterpret_cast<int*>(part + kTelThreads);              // [P][M]
  const int t = threadIdx.x, ml = t % M, js = t / M;
  const int mode = mb * M + ml;
  const bool live = mode < a.A;
  const size_t bm = (size_t)b * a.A + mode;

  const double* hist = reinterpret_cast<const double*>(a.state + (size_t)b * a.rec_bytes);
  const long long* cs = reinterpret_cast<const long long*>(hist + (size_t)a.T * a.A);
  const long long count = cs[0];
  const int n = count < 0 ? 0 : (count < (long long)a.T ? (int)count : a.T);
  if (n < S) {   // not one segment yet: NaN rows, 0 segments
    const double nan = __builtin_nan("");
    if (a.psd)
      for (int idx = t; idx < M * NB; idx += kTelThreads) {
        const int mm = idx / NB;
        if (mb * M + mm < a.A) a.psd[((size_t)b * a.A + mb * M) * NB + idx] = nan;
      }
    if (a.segments && mb == 0 && t == 0) a.segments[b] = 0;
    if (a.r2 && js == 0 && live) {
      a.gain[bm] = nan;
      a.cost[bm] = nan;
      if (a.cost_all)
        for (int g = 0; g < a.G; ++g) a.cost_all[bm * a.G + g] = nan;
    }
    return;
  }
  const int nseg = (n - S) / H + 1;
  const int row0 = (int)((count - (long long)((nseg - 1) * H + S)) & (long long)(a.T - 1));   // the oldest row that enters

  for (int q = t; q < H; q += kTelThreads) {
    double s, c;
    sincospi(2.0 * (double)q / (double)S, &s, &c);
    tw[q] = make_double2(c, -s);
  }

  // the thread's E rows of half segment h; the seam of the ring from one workgroup-uniform number
  const auto load_half = [&](int h, double (&v)[E]) {
    const int start = (row0 + h * H) & (a.T - 1);
    const int wrap = a.T - start;   // rows before the seam
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int r = js + i * P;
      const int row = r < wrap ? start + r : r - wrap;
      v[i] = live ? hist[(size_t)row * a.A + mode] : 0.0;
    }
  };

  double prev[E], cur[E], acc[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) acc[i] = 0.0;
  load_half(0, prev);
  for (int s = 0; s < nseg; ++s) {
    load_half(s + 1, cur);
    double ps = prev[0];
#pragma unroll
    for (int i = 1; i < E; ++i) ps = ps + prev[i];
#pragma unroll
    for (int i = 0; i < E; ++i) ps = ps + cur[i];
    part[js * M + ml] = ps;
    __syncthreads();   // part (and, the first time, tw)
    double mean = part[ml];
#pragma unroll
    for (int q = 1; q < P; ++q) mean = mean + part[q * M + ml];
    mean = mean / (double)S;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int r = js + i * P;   // < S / 2
      const double c = tw[r].x;   // cos(2 pi r / S); row r + S / 2 has the opposite sign
      const size_t at = ((size_t)(r >> 1) * M + ml) * 2 + (r & 1);
      workd[at] = (prev[i] - mean) * (0.5 * (1.0 - c));
      workd[at + (size_t)(H / 2) * M * 2] = (cur[i] - mean) * (0.5 * (1.0 + c));
      prev[i] = cur[i];
    }
    __syncthreads();
    for (int half = N / 2; half >= 1; half >>= 1) {
      const int tstep = N / half;
#pragma unroll
      for (int u = 0; u < BF; ++u) {
        const int j = js + u * P;
        const int pos = j & (half - 1);
        const int i0 = ((j - pos) << 1) + pos;
        const double2 x0 = work[(size_t)i0 * M + ml], x1 = work[(size_t)(i0 + half) * M + ml];
        const double2 w = tw[pos * tstep];
        const double dx = x0.x - x1.x, dy = x0.y - x1.y;
        work[(size_t)i0 * M + ml] = make_double2(x0.x + x1.x, x0.y + x1.y);
        work[(size_t)(i0 + half) * M + ml] = make_double2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k = js + i * P;
      if (k <= H) {
        const int k1 = k & (N - 1), k2 = (N - k) & (N - 1);
        const double2 z1 = work[(size_t)(__brev((unsigned)k1) >> (32 - Geo::LOGN)) * M + ml];
        const double2 z2 = work[(size_t)(__brev((unsigned)k2) >> (32 - Geo::LOGN)) * M + ml];
        const double ex = 0.5 * (z1.x + z2.x), ey = 0.5 * (z1.y - z2.y);
        const double ox = 0.5 * (z1.y + z2.y), oy = -0.5 * (z1.x - z2.x);
        const double2 w = k < N ? tw[k] : make_double2(-1.0, 0.0);
        const double xr = ex + (w.x * ox - w.y * oy), xi = ey + (w.x * oy + w.y * ox);
        acc[i] = acc[i] + (xr * xr + xi * xi);
      }
    }
    __syncthreads();   // the transform's last readers, before the next segment or Phi overwrites it
  }

  // Phi [k][M + 1] in the transform's words
  const double norm = 0.375 * (double)S * (double)S;
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const int k = js + i * P;
    if (k <= H) workd[(size_t)k * (M + 1) + ml] = (((k == 0 || k == H) ? 1.0 : 2.0) * (acc[i] / (double)nseg)) / norm;
  }
  __syncthreads();
  if (a.psd)
    for (int idx = t; idx < M * NB; idx += kTelThreads) {
      const int mm = idx / NB, k = idx - mm * NB;
      if (mb * M + mm < a.A) a.psd[((size_t)b * a.A + mb * M) * NB + idx] = workd[(size_t)k * (M + 1) + mm];
    }
  if (a.segments && mb == 0 && t == 0) a.segments[b] = nseg;
  if (!a.r2) return;

  // the gains: thread (js, m) the candidates js, js + P, ..., its first minimiser; then the P of a mode in grid order
  double best = 0.0;
  int best_g = -1;
  for (int g = js; g < a.G; g += P) {
    const double* r2 = a.r2 + (size_t)g * H;
    double J = 0.0;
    for (int k = 1; k <= H; ++k) J = J + r2[k - 1] * workd[(size_t)k * (M + 1) + ml];
    if (a.cost_all && live) a.cost_all[bm * a.G + g] = J;
    if (best_g < 0 || J < best) {
      best = J;
      best_g = g;
    }
  }
  part[js * M + ml] = best;
  cand[js * M + ml] = best_g;
  __syncthreads();
  if (js == 0 && live) {   // (slot 0 holds candidate 0: there is always one)
    for (int q = 1; q < P; ++q) {
      const double J = part[q * M + ml];
      const int g = cand[q * M + ml];
      if (g >= 0 && (J < best || (J == best && g < best_g))) {
        best = J;
        best_g = g;
      }
    }
    a.gain[bm] = a.r2[(size_t)a.G * H + best_g];
    a.cost[bm] = best;
  }
}

}  // namespace aog
