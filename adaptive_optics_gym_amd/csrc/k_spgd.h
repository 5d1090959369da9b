// K19: stochastic parallel gradient descent (SPGD), the sensorless baseline (aog_spgd_*, aog_reset_spgd / aog_step_spgd): the query one wave
// runs for one env.  k_spgd_update (spgd.hip) is the stand-alone kernel around it, k_epilogue_spgd_prologue (k_step_spgd.h) the fused step tail.
#pragma once
#include "k_common.h"

namespace aog {

// Per env one record of A + 2 doubles: the centre command u [A], J_plus, then k and h as two uint32 in the last 8 bytes.
// Two-sided SPGD with Bernoulli perturbations: delta_k in {-1, +1}^A, bit i & 31 of word (i >> 5) & 3 of the Philox4x32-10 call with
// counter (global env id, k, i >> 7, kSpgdTag) keyed by the controller's seed; a set bit is +1.
//   query, h = 0: the command in place gave J:  J_plus = J,  emit u - amplitude delta_k,  h = 1
//   query, h = 1: u = clip(u + (gain (J_plus - J)) delta_k),  k += 1,  h = 0,  emit u + amplitude delta_k (the new k's)
//   reset:        u = 0 (or the row of `start`),  h = 0,  k kept,  emit u + amplitude delta_k
// J is a float32 widened; every product and sum is one rounded float64 operation (__dmul_rn / __dadd_rn: nothing is contracted), the
// emitted command is the float32 of the float64 sum: a host replay from the recorded J is bit-exact.
constexpr uint32_t kSpgdTag = 0x53504744u;   // "SPGD": the stream tag, word 3 of the counter
constexpr int kSpgdEnvs = 4;                 // envs (= waves) per workgroup of the stand-alone kernel
struct SpgdArgs {
  double* state;            // [B] records
  const double* gain;       // [B]
  const double* amplitude;  // [B]
  const float* metric;      // [B]; unused by a reset
  const uint8_t* mask;      // nullable [B]: envs it leaves out keep their state and their row of `action`
  const double* start;      // reset: nullable [B][A] actuators to start from
  float* action;            // [B][A] the emitted command; nullable in a stand-alone reset
  int B, A, env_base, reset;
  uint32_t seed_lo, seed_hi;
  double clip;              // 0: no bound
};
__host__ __device__ inline size_t spgd_record_doubles(int A) { return (size_t)A + 2; }

// The 64 words of calls 16 r .. 16 r + 15 of (env, k): lane L forms call 16 r + (L >> 2) and keeps its word L & 3, so the word of actuator
// i (2048 r <= i < 2048 r + 2048) lies in lane (i >> 5) & 63 — one Philox evaluation per wave and 2048 actuators, handed out by
// ds_bpermute (spgd_sign).
__device__ __forceinline__ uint32_t spgd_words(const SpgdArgs& s, uint32_t genv, uint32_t k, int r, int lane) {
  uint32_t c[4] = {genv, k, (uint32_t)(16 * r + (lane >> 2)), kSpgdTag};
  uint32_t k0 = s.seed_lo, k1 = s.seed_hi;
#pragma unroll
  for (int rr = 0; rr < 10; ++rr) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t lo = (lane & 1) ? c[1] : c[0], hi = (lane & 1) ? c[3] : c[2];
  return (lane & 2) ? hi : lo;
}
// delta of actuator i as +-1.0 from the wave's words (every lane of the wave calls this together)
__device__ __forceinline__ double spgd_sign(uint32_t words, int i) {
  const uint32_t w = (uint32_t)__shfl((int)words, (i >> 5) & 63, 64);
  return ((w >> (i & 31)) & 1u) ? 1.0 : -1.0;
}

// One query (or reset) of env `env` by one whole wave; lanes stride the actuators.  The trip counts are uniform over the wave: the
// shuffles see all 64 lanes.
__device__ __forceinline__ void spgd_query(const SpgdArgs& s, int env, int lane) {
  const int A = s.A;
  double* __restrict__ rec = s.state + (size_t)env * spgd_record_doubles(A);
  uint32_t* kh = reinterpret_cast<uint32_t*>(rec + A + 1);
  const uint32_t k = kh[0], h = kh[1];
  const uint32_t genv = (uint32_t)(s.env_base + env);
  const double amp = s.amplitude[env];
  float* __restrict__ out = s.action ? s.action + (size_t)env * A : nullptr;
  const bool first_half = !s.reset && h == 0;
  const bool second_half = !s.reset && h != 0;
  double step = 0.0;   // gain (J_plus - J)
  if (!s.reset) {
    const double J = (double)s.metric[env];
    if (second_half) step = __dmul_rn(s.gain[env], __dadd_rn(rec[A], -J));
    else if (lane == 0) rec[A] = J;
  }
  const uint32_t k_emit = second_half ? k + 1u : k;
  const double side = first_half ? -amp : amp;
  for (int base = 0; base < A; base += 2048) {
    const int r = base >> 11;
    const uint32_t w_emit = spgd_words(s, genv, k_emit, r, lane);
    const uint32_t w_old = second_half ? spgd_words(s, genv, k, r, lane) : 0u;
    for (int i0 = base; i0 < min(A, base + 2048); i0 += 64) {
      const int i = i0 + lane;
      const double d_emit = spgd_sign(w_emit, i);
      const double d_old = second_half ? spgd_sign(w_old, i) : 0.0;
      if (i < A) {
        double u;
        if (s.reset) {
          u = s.start ? s.start[(size_t)env * A + i] : 0.0;
          rec[i] = u;
        } else {
          u = rec[i];
          if (second_half) {
            u = __dadd_rn(u, __dmul_rn(step, d_old));
            if (s.clip > 0.0) u = u > s.clip ? s.clip : (u < -s.clip ? -s.clip : u);
            rec[i] = u;
          }
        }
        if (out) out[i] = (float)__dadd_rn(u, __dmul_rn(side, d_emit));
      }
    }
  }
  if (lane == 0) {
    kh[0] = k_emit;
    kh[1] = first_half ? 1u : 0u;
  }
}

}  // namespace aog
