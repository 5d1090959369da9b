// The photon-count sampler shared by the Shack-Hartmann camera (k_shack.h) and the photodetector model of the observations (k_detector.h):
// one definition, so that both draw the same law from the same words.
#pragma once
#include "k_common.h"

namespace aog {

// hcipy.util.large_poisson with the handle's Philox stream: exact inversion for lambda < 12, above it the rounded normal approximation with the
// Cornish-Fisher skewness term (hcipy switches to a plain rounded normal at 1e6; the sensor's controller reads flux-weighted centroids
// of ~1e3 pixels per lenslet: mean, variance and third moment of every pixel's count are those of the Poisson law).
// Stream layout: with x = l + LW r (LW = 64, or 60 for pupils of 60 R pixels: spectrum_lane_width), pixel (global env ge, row y, column x)
// takes word r & 3 of the Philox call with counter ((ge N + y) 64 + l, group r >> 2, call) — and, when it is bright, the same word of a second call for the Box-Muller angle.  The
// lane of the fused row pass that holds columns x, x + 64, x + 128, ... therefore draws ONE call per four of its pixels (a call per pixel
// with a float64 exp and a float64 inversion was ~350 instructions per pixel: two thirds of that pass); results do not depend on the
// batch split, nor on which kernel draws them.
__device__ __forceinline__ void sh_noise_words(size_t line, uint32_t group, bool second, unsigned long long seed, uint32_t call, uint32_t (&w)[4]) {
  uint32_t c[4] = {(uint32_t)line, (uint32_t)(line >> 32) ^ (group << 20) ^ (second ? 0x80000000u : 0u), call, 0x50155u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  w[0] = c[0]; w[1] = c[1]; w[2] = c[2]; w[3] = c[3];
}
constexpr double kShPoissonSwitch = 12.0;
// Poisson(lam), lam < 12, by inversion on a 32-bit uniform: k = number of partial sums of the pmf that stay below u.  The wave walks the
// terms in lockstep (k is wave-uniform, 1 / k is an immediate), FOUR terms per round of the "is any lane still below its u" vote, in fp32:
// the pmf recurrence p_k = p_{k-1} lam / k and its running sum carry ~1e-6 relative error, i.e. the sampled law differs from Poisson(lam)
// by ~1e-6 in total variation (the uniform is shrunk by 4e-6 so that the accumulated distribution always reaches it) — three orders
// below what a chi-square test on 1e6 draws resolves (tests: test_device_poisson_sampler_matches_scipy).  Round 2's form (float64 terms,
// one vote per term) spent ~70 cycles per term and was half of the fused row pass; this one spends ~25.  At most 48 terms: P(k > 47 | 12) < 1e-14.
template <int K0>
__device__ __forceinline__ void sh_poisson_terms(float lam, float u, float& pk, float& cdf, int& kres) {
  if (!__any(u > cdf ? 1 : 0)) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    kres += u > cdf ? 1 : 0;                   // (the sum only grows: once u <= cdf the lane stops counting)
    pk *= lam * (1.0f / (float)(K0 + j));      // compile-time reciprocal
    cdf += pk;
  }
  if constexpr (K0 + 4 < 48) sh_poisson_terms<K0 + 4>(lam, u, pk, cdf, kres);
}
__device__ __forceinline__ double sh_poisson_small(double lam_d, uint32_t word, bool active) {
  const float lam = (float)lam_d;
  const float u = active ? ((float)(word >> 8) + 0.5f) * (1.0f / 16777216.0f) * (1.0f - 4e-6f) : 0.0f;
  float pk = __expf(-lam), cdf = pk;
  int kres = 0;
  sh_poisson_terms<1>(lam, u, pk, cdf, kres);
  return (double)kres;
}
// rounded normal approximation with the Cornish-Fisher skewness term (matches mean, variance and third moment of Poisson(lam))
__device__ __forceinline__ double sh_poisson_large(double lam, uint32_t word_r, uint32_t word_a) {
  const float u1 = ((float)(word_r >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = (float)(word_a >> 8) * (1.0f / 16777216.0f);   // revolutions
  const float g = sqrtf(-2.0f * __logf(u1)) * __builtin_amdgcn_cosf(u2);
  return fmax(0.0, rint(lam + (double)(g * sqrtf((float)lam) + (g * g - 1.0f) * (1.0f / 6.0f))));
}

}  // namespace aog
