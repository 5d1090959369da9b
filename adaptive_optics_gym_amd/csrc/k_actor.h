// R1: policy query of the rollout: the device building blocks (kernel k_actor_act in actor.hip, the fused step tail in k_step_act.h).
#pragma once
#include "k_common.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// R1  policy query of the rollout (network.py:48-69): a 3-hidden-layer ReLU MLP with active dropout, Gaussian action sampling
// and its log-probability, one launch.  Workgroup = 16 envs (the 16 columns of v_mfma_f32_16x16x4_f32, exact fp32), 4 waves
// share the output-unit tiles of a layer; activations [unit][16 envs] ping-pong in LDS; nn.Linear weights [out][in] are read
// straight from global memory as the A operand (lane = unit % 16 + 16 (k % 4)).
// ------------------------------------------------------------------------------------------------
// aog_action_noise as the kernels read it (ActorNoiseArgs: k_actor_act_noise / k_epilogue_act_prologue_noise only; the plain kernels keep
// their arguments and code): mode 0 = the sampled action, 1 = the mean (no eps); ou = the caller's Ornstein-Uhlenbeck state [B][A] float64,
// nullptr = no OU term
struct ActorNoise {
  int mode;
  double* ou;
  double mu, theta, sigma;
};
struct ActorArgs {
  const void* obs;
  const float *w1, *b1, *w2, *b2, *w3, *b3, *wo, *bo;
  float *mean, *action, *log_prob;
  int B, S, H, A, obs_f16, kpad;
  int kpad_b, wfloats;   // rows of the hidden-only activation buffer xb; LDS floats of a weight chunk (<= kActorWFloats)
  float p_drop, keep_scale, std, logp_const;
  unsigned long long seed;
  uint32_t call_lo, call_hi;
  int env_base;   // global id of obs row 0
};
struct ActorNoiseArgs : ActorArgs {
  ActorNoise nz;
};
__device__ __forceinline__ void actor_philox(uint32_t (&c)[4], unsigned long long seed) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// out[m][e] = act(sum_k W[m][k] xin[k][e] + b[m]) for this workgroup's 16 envs; LAYER 1..3 hidden (relu + dropout), 4 output.
// The weights cross HBM/L2 -> registers -> LDS one row chunk at a time as a linear 16-byte-per-lane copy (every load of the chunk in
// flight at once: one memory round trip), and the NEXT chunk — of this layer or the first of the following layer — is requested
// before the matrix work on the current one starts, so the round trips of the four layers hide behind each other's arithmetic
// (the kernel is one latency chain: 64 workgroups at B = 1024, 220 KB of weights each).
constexpr int kActorWFloats = 24576;   // LDS floats for a weight chunk (96 KB)
constexpr int kActorThreads = 640;     // 10 waves: one 16-unit tile each for the reference's 150 hidden units
constexpr int kActorPre = 10;          // float4 registers per thread holding a chunk in flight (640 x 10 x 4 >= kActorWFloats)
// THREADS (a multiple of 64) threads share a layer's tiles and PRE float4 registers each hold the chunk in flight (THREADS x PRE x 4 >= the
// chunk's floats): k_actor_act runs <kActorThreads, kActorPre>, the fused step tail (k_step_act.h) its own 1024-thread shape.  A tile's
// accumulation chain is the same whichever wave runs it.
// One OU step in the reference's order of operations (network.py:268-272, float64): dx = theta (mu - s) + sigma n, s + dx.  No fused
// multiply-add, as numpy computes it.
__device__ __forceinline__ double ou_advance(double s, double mu, double theta, double sigma, float n) {
#pragma clang fp contract(off)
  const double dx = theta * (mu - s) + sigma * (double)n;
  return s + dx;
}
__device__ __forceinline__ int actor_rows_max(int K, int wfloats) { return max(16, ((wfloats / K) >> 4) << 4); }
// request rows [r0, r0 + rows_max) of W ([M][K], 16-byte aligned base; r0 is a multiple of 16)
template <int THREADS, int PRE>
__device__ __forceinline__ void actor_issue(f32x4 (&pre)[PRE], const float* __restrict__ W, int K, int M, int r0, int wfloats) {
  const int rc = min(actor_rows_max(K, wfloats), M - r0);
  const int n4 = (rc * K) >> 2;
  const f32x4* src = reinterpret_cast<const f32x4*>(W + (size_t)r0 * K);
#pragma unroll
  for (int u = 0; u < PRE; ++u) pre[u] = src[min((int)threadIdx.x + THREADS * u, max(n4 - 1, 0))];
}
// NOISE (layer 4 only, P = ActorNoiseArgs): the output stage applies p.nz (mean mode, OU term); without it the code is that of the plain query.
template <int LAYER, int THREADS, int PRE, bool NOISE = false, class P = ActorArgs>
__device__ __forceinline__ void actor_layer(const P& p, const float* __restrict__ W, const float* __restrict__ bias, int K, int M,
                                            const float* xin, float* xout, float* lp_sum, float* wl, int env0, f32x4 (&pre)[PRE],
                                            const float* __restrict__ Wnext, int Knext, int Mnext, int kin, int kout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int el = lane & 15, kq = lane >> 4;
  const int n_steps = (K + 3) >> 2;
  const int rows_max = actor_rows_max(K, p.wfloats);
  for (int r0 = 0; r0 < M; r0 += rows_max) {
    const int rc = min(rows_max, M - r0);
    const int n_fl = rc * K;
    const float* src = W + (size_t)r0 * K;   // 16-byte aligned: r0 is a multiple of 16 and the base pointer is (checked on the host)
    {
      // `pre` holds this chunk (requested during the previous chunk's matrix work, or at kernel start)
      const int n4 = n_fl >> 2;
#pragma unroll
      for (int u = 0; u < PRE; ++u)
        if ((int)threadIdx.x + THREADS * u < n4) reinterpret_cast<f32x4*>(wl)[threadIdx.x + THREADS * u] = pre[u];
      for (int i = (n4 << 2) + threadIdx.x; i < n_fl; i += THREADS) wl[i] = src[i];
    }
    __syncthreads();
    if (r0 + rows_max < M) actor_issue<THREADS, PRE>(pre, W, K, M, r0 + rows_max, p.wfloats);
    else if (Wnext != nullptr) actor_issue<THREADS, PRE>(pre, Wnext, Knext, Mnext, 0, p.wfloats);
    __builtin_amdgcn_sched_barrier(0);   // (keep the requests ahead of the matrix work)
    const int n_tiles = (rc + 15) >> 4;
    for (int tile = wave; tile < n_tiles; tile += THREADS / 64) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int lrow = tile * 16 + el;                 // row inside the chunk
      const float row_ok = lrow < rc ? 1.f : 0.f;
      const float* wrow = wl + (size_t)min(lrow, rc - 1) * K;
      // D: column = env (lane & 15), rows 4 (lane >> 4) + r.  The biases (a global-memory round trip) and the random words of this
      // tile do not depend on the products: both are started before the matrix loop
      const int m0 = r0 + tile * 16 + 4 * kq;
      const int env = env0 + el;
      float bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = bias[min(m0 + r, M - 1)];
      uint32_t c[4] = {(uint32_t)m0 | ((uint32_t)LAYER << 24), (uint32_t)(p.env_base + env), p.call_lo, p.call_hi ^ 0xAC70u};
      actor_philox(c, p.seed);
      // OU term: the state of this tile's (env, unit)s and its normals (layer tag 5: a stream of its own, independent of the dropout masks
      // and of eps) are started before the matrix loop too
      constexpr bool kOu = LAYER == 4 && NOISE;
      double sv[4] = {0.0, 0.0, 0.0, 0.0};
      uint32_t cn[4] = {0u, 0u, 0u, 0u};
      if constexpr (kOu) {
        if (p.nz.ou != nullptr) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (m0 + r < M && env < p.B) sv[r] = p.nz.ou[(size_t)env * M + m0 + r];
          cn[0] = (uint32_t)m0 | (5u << 24); cn[1] = (uint32_t)(p.env_base + env); cn[2] = p.call_lo; cn[3] = p.call_hi ^ 0xAC70u;
          actor_philox(cn, p.seed);
        }
      }
      // Eight k-steps at a time: their 16 LDS reads are in flight together and the matrix ops follow back to back.  Whole groups
      // below K need no clamps or masks (rows past the chunk are clamped to a valid row and dropped at the output), so their reads
      // are base + immediate offset and the loop is the matrix pipe's: three waves share a SIMD's, and with ~15 address/mask
      // instructions per step the vector unit, not the matrix pipe, set the pace (timeline: 5.9 us per 150 x 150 layer).
      const int n_full = (K >> 2) & ~7;   // k-steps in whole unmasked groups
      {
        const float* wa = wrow + kq;
        const float* xb = xin + kq * 16 + el;
        for (int s0 = 0; s0 < n_full; s0 += 8, wa += 32, xb += 8 * 64) {
          float av[8], xv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            av[u] = wa[4 * u];
            xv[u] = xb[64 * u];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], xv[u], acc, 0, 0, 0);
        }
      }
      for (int s0 = n_full; s0 < n_steps; s0 += 8) {
        float av[8], xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = 4 * (s0 + u) + kq;
          av[u] = wrow[min(k, K - 1)] * (k < K ? row_ok : 0.f);
          xv[u] = xin[min(k, kin - 1) * 16 + el];   // rows K .. kin-1 of xin are zero; steps past the end multiply by a = 0
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], xv[u], acc, 0, 0, 0);
      }
      if constexpr (LAYER < 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + r;
          float v = 0.f;
          if (m < M) {
            v = fmaxf(acc[r] + bv[r], 0.f);
            const float u = (float)(c[r] >> 8) * (1.0f / 16777216.0f);   // [0, 1): keep with probability 1 - p
            v = u >= p.p_drop ? v * p.keep_scale : 0.f;
          }
          if (m < kout) xout[m * 16 + el] = v;   // units M .. are written as zero: the next layer's K padding
        }
      } else {
        float ssq = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float u1 = ((float)c[2 * h] + 0.5f) * (1.0f / 4294967296.0f), u2 = ((float)c[2 * h + 1] + 0.5f) * (1.0f / 4294967296.0f);
          const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
          const float eps[2] = {rad * __builtin_amdgcn_cosf(u2), rad * __builtin_amdgcn_sinf(u2)};
          float on[2] = {0.f, 0.f};   // the OU normals: eps's Box-Muller form on the tag-5 words
          if constexpr (kOu) {
            const float w1 = ((float)cn[2 * h] + 0.5f) * (1.0f / 4294967296.0f), w2 = ((float)cn[2 * h + 1] + 0.5f) * (1.0f / 4294967296.0f);
            const float rn = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(w1));
            on[0] = rn * __builtin_amdgcn_cosf(w2);
            on[1] = rn * __builtin_amdgcn_sinf(w2);
          }
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int m = m0 + 2 * h + t;
            if (m < M && env < p.B) {
              const float mu = acc[2 * h + t] + bv[2 * h + t];
              if (p.mean) p.mean[(size_t)env * M + m] = mu;
              if constexpr (NOISE) {
                // mean mode: the action is the mean and log_prob the density there (-logp_const: no eps enters)
                float g = mu;
                if (p.nz.mode == 0) {
                  g = mu + p.std * eps[t];
                  ssq += eps[t] * eps[t];
                }
                if (p.nz.ou != nullptr) {   // numpy's float32 += float64: the sum in float64, rounded once
                  const double s = ou_advance(sv[2 * h + t], p.nz.mu, p.nz.theta, p.nz.sigma, on[t]);
                  p.nz.ou[(size_t)env * M + m] = s;
                  g = (float)((double)g + s);
                }
                if (p.action) p.action[(size_t)env * M + m] = g;
              } else {
                if (p.action) p.action[(size_t)env * M + m] = mu + p.std * eps[t];
                ssq += eps[t] * eps[t];
              }
            }
          }
        }
        atomicAdd(&lp_sum[el], ssq);
      }
    }
    __syncthreads();   // the chunk is consumed before the next one (or the next layer's) overwrites wl
  }
}

// LDS of a policy query: xa [kpad][16] | xb [kpad_b][16] | lp [16] | weight chunk [wfloats] (xa: the observations, then layer 2's output;
// xb: the outputs of layers 1 and 3).  actor_act_floats = the floats before the chunk.
__host__ __device__ inline size_t actor_act_floats(int kpad, int kpad_b) { return (size_t)(kpad + kpad_b) * 16 + 16; }
// The four layers and the log-probability of this workgroup's 16 envs (env0 ..), the observations staged in xa, the first weight chunk of
// layer 1 in flight in `pre`.  Ends with a barrier: the LDS is free afterwards.
template <int THREADS, int PRE, bool NOISE = false, class P = ActorArgs>
__device__ __forceinline__ void actor_mlp(const P& p, float* lds_act, int env0, f32x4 (&pre)[PRE]) {
  float* xa = lds_act;
  float* xb = xa + (size_t)p.kpad * 16;
  float* lp = xb + (size_t)p.kpad_b * 16;
  float* wt = lp + 16;
  actor_layer<1, THREADS, PRE, false, P>(p, p.w1, p.b1, p.S, p.H, xa, xb, lp, wt, env0, pre, p.w2, p.H, p.H, p.kpad, p.kpad_b);
  __syncthreads();
  actor_layer<2, THREADS, PRE, false, P>(p, p.w2, p.b2, p.H, p.H, xb, xa, lp, wt, env0, pre, p.w3, p.H, p.H, p.kpad_b, p.kpad);
  __syncthreads();
  actor_layer<3, THREADS, PRE, false, P>(p, p.w3, p.b3, p.H, p.H, xa, xb, lp, wt, env0, pre, p.wo, p.H, p.A, p.kpad, p.kpad_b);
  __syncthreads();
  actor_layer<4, THREADS, PRE, NOISE, P>(p, p.wo, p.bo, p.H, p.A, xb, nullptr, lp, wt, env0, pre, nullptr, 0, 0, p.kpad_b, 0);
  __syncthreads();
  if (threadIdx.x < 16 && env0 + threadIdx.x < p.B && p.log_prob) p.log_prob[env0 + threadIdx.x] = -0.5f * lp[threadIdx.x] - p.logp_const;
  __syncthreads();
}

}  // namespace aog
