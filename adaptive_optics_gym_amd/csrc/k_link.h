// K20: link telemetry (aog_link_*): a ring of the fibre-coupled power per env, and over what the ring holds the figures a free-space
// optical link is judged by — fade probability, fade count and duration per threshold, the power histogram, the scintillation index's
// two moments and the mean bit-error rate of on-off keying.  Float64 accumulators without fused multiply-add, plain vector stores, no
// atomics on floats (the histogram's int32 counters are LDS atomics: integer sums have no order).
//
// Per env the handle keeps ONE record of 4 T + 16 bytes: ring [T] float32 (sample number c at c mod T), then count and skipped as int64.
// The records of a handle lie one behind the other: that array is the state blob of aog_link_get_state.
//
// k_link_statistics — one wave per env, kLinkEnvs envs per workgroup (K19's shape: the work of an env is a few thousand samples, far too
// little for a workgroup, and a wave needs no barrier to combine its lanes).  The wave reads its ring once, in 16-byte pieces, and lays
// the window out in the LDS in CHRONOLOGICAL order (the ring's physical wrap is resolved here and nowhere else); everything else reads
// that copy.  Lane l owns the contiguous chunk [l C, (l + 1) C) of the window, C = T / 64; sample i lies at word i + i / C, so that the
// lanes' chunk walks (stride C + 1 words, odd) fall on distinct banks.
//   pass 1   per lane, in chunk order: sum p, sum p^2 (the square of a float32 is exact in float64), min, max; across lanes a 6-step
//            xor butterfly, whose result is the same bits in every lane.  mean = sum / n, and with it the reference level P.
//   edges    lane j: P g_j into the LDS; the E + 1 counters zeroed.
//   bins     per sample the number of edges <= p by bisection (<= 7 LDS reads), one int32 LDS atomic per sample.
//   fades    per threshold k, edge P f_k: the lane reduces its chunk to a segment summary (length, below, runs, prefix run, suffix run,
//            longest run; all_below is below == length) and the 64 summaries are merged in lane order by a 6-step tree (lane l takes
//            lane l + 2^s as its RIGHT neighbour): two runs that touch fuse into one, longest takes left.suffix + right.prefix into
//            account, an empty segment is the identity.  A 200-frame fade over whole all-below lanes is just that merge.
//   BER      per Q factor: erfc((q / (P sqrt 2)) p) summed per lane in chunk order, the butterfly, / (2 n).
// The chunking depends on T alone and the sums' order on (T, n) alone — never on the batch, the mask or the env's place in a workgroup:
// a split batch reproduces the whole one bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aog {

constexpr int kLinkMinT = 64, kLinkMaxT = 4096;
constexpr int kLinkMaxK = 16, kLinkMaxE = 64, kLinkMaxQ = 8;   // thresholds, histogram edges, Q factors (AOG_LINK_MAX_*)
constexpr int kLinkEnvs = 4;                                   // envs (= waves) per workgroup of k_link_statistics
constexpr int kLinkBinWords = kLinkMaxE + 4;                   // the counters' words of a wave (E + 1 used)

struct LinkArgs {
  char* state;           // [B] records
  size_t rec_bytes;
  const uint8_t* mask;   // nullable [B]
  int B, T;
  const float* power;    // push: [B]
};

struct LinkStatArgs {
  LinkArgs h;
  int mean_reference;    // 1: P = the env's mean; 0: P = reference
  int K, E, Q;
  double reference;
  double f[kLinkMaxK], g[kLinkMaxE], q[kLinkMaxQ];
  int* samples;          // [B]
  double* mean;          // [B]
  double* mean_square;   // [B]
  float* minimum;        // [B]
  float* maximum;        // [B]
  double* level;         // [B] the reference level P
  int* below;            // [B][K]
  int* fades;            // [B][K]
  int* longest;          // [B][K]
  int* hist;             // [B][E + 1]
  double* ber;           // [B][Q]
};

__host__ __device__ inline size_t link_record_bytes(int T) { return (size_t)T * sizeof(float) + 2 * sizeof(long long); }
// a wave's LDS: the histogram edges [kLinkMaxE] float64, the window [T + 64] float32 (one pad word per chunk), the counters
__host__ __device__ inline size_t link_wave_lds_bytes(int T) {
  return kLinkMaxE * sizeof(double) + ((size_t)T + 64) * sizeof(float) + kLinkBinWords * sizeof(int);
}

__device__ inline bool link_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }

// one sample per selected env into its ring; a non-finite one is counted in `skipped` instead
__global__ __launch_bounds__(256) void k_link_push(LinkArgs a) {
  const int b = (int)(blockIdx.x * 256 + threadIdx.x);
  if (b >= a.B || (a.mask && !a.mask[b])) return;
  float* ring = reinterpret_cast<float*>(a.state + (size_t)b * a.rec_bytes);
  long long* cs = reinterpret_cast<long long*>(ring + a.T);
  const float v = a.power[b];
  if (!link_finite(v)) {
    cs[1] = cs[1] + 1;
    return;
  }
  const long long cnt = cs[0];
  ring[(int)(cnt & (long long)(a.T - 1))] = v;
  cs[0] = cnt + 1;
}

// the state after create: an empty ring of zeros, both counters 0
__global__ __launch_bounds__(256) void k_link_reset(LinkArgs a) {
  const int b = blockIdx.x;
  if (a.mask && !a.mask[b]) return;
  float* ring = reinterpret_cast<float*>(a.state + (size_t)b * a.rec_bytes);
  long long* cs = reinterpret_cast<long long*>(ring + a.T);
  for (int i = threadIdx.x; i < a.T; i += 256) ring[i] = 0.f;
  if (threadIdx.x < 2) cs[threadIdx.x] = 0;
}

__device__ __forceinline__ double link_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// A stretch of the window reduced for one threshold.  all_below is below == length; the empty stretch is the merge's identity.
struct LinkSegment {
  int length, below, runs, prefix, suffix, longest;
};
// `l` then `r`, in chronological order
__device__ __forceinline__ LinkSegment link_merge(const LinkSegment& l, const LinkSegment& r) {
  LinkSegment m;
  m.length = l.length + r.length;
  m.below = l.below + r.below;
  m.runs = l.runs + r.runs - ((l.suffix > 0 && r.prefix > 0) ? 1 : 0);
  m.prefix = l.below == l.length ? l.length + r.prefix : l.prefix;
  m.suffix = r.below == r.length ? r.length + l.suffix : r.suffix;
  m.longest = max(max(l.longest, r.longest), l.suffix + r.prefix);
  return m;
}

__global__ __launch_bounds__(64 * kLinkEnvs) void k_link_statistics(LinkStatArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char lds_link[];
  const int w = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int env = (int)blockIdx.x * kLinkEnvs + w;
  const int T = a.h.T, K = a.K, E = a.E, Q = a.Q;
  char* mine = lds_link + (size_t)w * link_wave_lds_bytes(T);
  double* edge = reinterpret_cast<double*>(mine);                                  // [kLinkMaxE]
  float* win = reinterpret_cast<float*>(mine + kLinkMaxE * sizeof(double));         // [T + 64]
  int* bins = reinterpret_cast<int*>(win + T + 64);                                 // [kLinkBinWords]
  const int C = T >> 6;                                      // samples of a lane's chunk
  const int pad_shift = C > 1 ? 31 - __clz(C) : 31;          // word of sample i: i + (i >> pad_shift)   (C = 1: no pad)
  const bool live = env < a.h.B && (!a.h.mask || a.h.mask[env]);   // (uniform per wave; every wave reaches the three barriers)

  int n = 0;
  if (live) {
    const float* ring = reinterpret_cast<const float*>(a.h.state + (size_t)env * a.h.rec_bytes);
    const long long count = *reinterpret_cast<const long long*>(ring + T);
    n = count < 0 ? 0 : (count < (long long)T ? (int)count : T);
    const int start = (int)((count - (long long)n) & (long long)(T - 1));   // where the oldest sample of the window lies (0 until the ring is full)
    const float4* ring4 = reinterpret_cast<const float4*>(ring);
    for (int j = lane; j < T / 4; j += 64) {
      if (n < T && 4 * j >= n) break;   // (a ring that is not full yet: nothing from here on)
      const float4 v = ring4[j];
      const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = (4 * j + c - start) & (T - 1);
        if (i < n) win[i + (i >> pad_shift)] = vs[c];
      }
    }
  }
  __syncthreads();   // the window

  const int lo = min(lane * C, n), hi = min(lane * C + C, n);   // the lane's chunk [lo, hi)
  double P = 0.0;
  if (live && n > 0) {
    double sum = 0.0, sq = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = lo; i < hi; ++i) {
      const float p = win[i + (i >> pad_shift)];
      const double pd = (double)p;
      sum = sum + pd;
      sq = sq + pd * pd;
      mn = fminf(mn, p);
      mx = fmaxf(mx, p);
    }
    sum = link_wave_sum(sum);
    sq = link_wave_sum(sq);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, off, 64));
      mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    const double mean = sum / (double)n;
    P = a.mean_reference ? mean : a.reference;
    if (lane == 0) {
      a.samples[env] = n;
      a.mean[env] = mean;
      a.mean_square[env] = sq / (double)n;
      a.minimum[env] = mn;
      a.maximum[env] = mx;
      a.level[env] = P;
    }
    if (lane < E) edge[lane] = P * a.g[lane];
    for (int j = lane; j <= E; j += 64) bins[j] = 0;
  }
  __syncthreads();   // the edges, the zeroed counters

  if (live && n > 0) {
    for (int i = lo; i < hi; ++i) {
      const double pd = (double)win[i + (i >> pad_shift)];
      int b0 = 0, b1 = E;   // the number of edges <= p lies in [b0, b1]
      while (b0 < b1) {
        const int mid = (b0 + b1) >> 1;
        if (pd >= edge[mid]) b0 = mid + 1;
        else b1 = mid;
      }
      atomicAdd(&bins[b0], 1);
    }
  }
  __syncthreads();   // the counters
  if (!live) return;

  if (n == 0) {   // an empty window: 0 in the integer outputs, NaN in the float ones
    const double nan = __builtin_nan("");
    if (lane == 0) {
      a.samples[env] = 0;
      a.mean[env] = nan;
      a.mean_square[env] = nan;
      a.minimum[env] = __builtin_nanf("");
      a.maximum[env] = __builtin_nanf("");
      a.level[env] = nan;
    }
    if (lane < K) {
      a.below[(size_t)env * K + lane] = 0;
      a.fades[(size_t)env * K + lane] = 0;
      a.longest[(size_t)env * K + lane] = 0;
    }
    for (int j = lane; j <= E; j += 64) a.hist[(size_t)env * (E + 1) + j] = 0;
    if (lane < Q) a.ber[(size_t)env * Q + lane] = nan;
    return;
  }

  for (int j = lane; j <= E; j += 64) a.hist[(size_t)env * (E + 1) + j] = bins[j];

  for (int k = 0; k < K; ++k) {
    const double e = P * a.f[k];
    LinkSegment s{hi - lo, 0, 0, 0, 0, 0};
    int cur = 0;
    bool leading = true;
    for (int i = lo; i < hi; ++i) {
      const bool in = (double)win[i + (i >> pad_shift)] < e;
      cur = in ? cur + 1 : 0;
      s.below += in ? 1 : 0;
      s.runs += (in && cur == 1) ? 1 : 0;
      s.longest = max(s.longest, cur);
      leading = leading && in;
      s.prefix += leading ? 1 : 0;
    }
    s.suffix = cur;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {   // lane l (a multiple of 2 off) holds lanes [l, l + off), lane l + off the next `off`
      LinkSegment r;
      r.length = __shfl_down(s.length, off, 64);
      r.below = __shfl_down(s.below, off, 64);
      r.runs = __shfl_down(s.runs, off, 64);
      r.prefix = __shfl_down(s.prefix, off, 64);
      r.suffix = __shfl_down(s.suffix, off, 64);
      r.longest = __shfl_down(s.longest, off, 64);
      s = link_merge(s, r);
    }
    if (lane == 0) {
      a.below[(size_t)env * K + k] = s.below;
      a.fades[(size_t)env * K + k] = s.runs;
      a.longest[(size_t)env * K + k] = s.longest;
    }
  }

  const double root2_P = P * 1.4142135623730951;
  for (int m = 0; m < Q; ++m) {
    const double scale = a.q[m] / root2_P;
    double acc = 0.0;
    for (int i = lo; i < hi; ++i) acc = acc + erfc(scale * (double)win[i + (i >> pad_shift)]);
    acc = link_wave_sum(acc);
    if (lane == 0) a.ber[(size_t)env * Q + m] = (0.5 * acc) / (double)n;
  }
}

}  // namespace aog
