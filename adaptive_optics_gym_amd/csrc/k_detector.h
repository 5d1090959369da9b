// Photodetector model of the observations (aog_set_detector): shot noise, read noise and a calibrated background on the focal-plane powers,
// applied where the step kernels store the observation (k_step.h, k_step_act.h, k_obs.h).  Handles without a detector never reach this code.
#pragma once
#include "k_poisson.h"

namespace aog {

// Per (global env ge, observation pixel j, frame): ONE Philox4x32-10 call keyed by the handle's rng_seed with counter
//   {j | kDetTag << 24,  ge,  frame & 0xFFFFFFFF,  (frame >> 32) ^ kDetFrameXor}
// word 0: the Poisson uniform (small branch) / Box-Muller radius (large branch), word 1: the large branch's angle, words 2, 3: radius and
// angle of the read-noise normal.  Word 3 of the counter tells the stream from the others under the same key: extrusion normals (0), screen
// synthesis (0x5C4EE7 / 8), Shack-Hartmann camera (0x50155), policy query (call_hi ^ 0xAC70, tags 1 .. 5 in word 0), pyramid sensor (frame_hi ^ 0x9F2A31D, k_pyramid.h).
constexpr uint32_t kDetTag = 6u;
constexpr uint32_t kDetFrameXor = 0xDE7EC7u;

struct DetectorArgs {
  const double* par;     // [3][B]: photons F_e, read noise sigma_e, background b_e
  const uint8_t* mask;   // nullable (masked reset): envs with mask[e] == 0 draw nothing and keep the observation they had
  unsigned long long seed;
  uint32_t frame_lo, frame_hi;
  int env_base, B;
};

// The noisy value of one pixel from its clean float64 power w.  Called by whole waves (`active` = this lane has a pixel): the small
// branch's inversion is a loop the wave walks together (sh_poisson_small).
//   c = double(float(w)), lam = F c + b, n = large_poisson(lam), y = (n + sigma g - b) / F      (float64, no fused multiply-add)
__device__ __forceinline__ double det_noisy_value(const DetectorArgs& d, double w, int env, int j, bool active) {
#pragma clang fp contract(off)
  const int el = active ? env : 0;
  const double F = d.par[el], sigma = d.par[d.B + el], b = d.par[2 * d.B + el];
  uint32_t c[4] = {(uint32_t)j | (kDetTag << 24), (uint32_t)(d.env_base + env), d.frame_lo, d.frame_hi ^ kDetFrameXor};
  uint32_t k0 = (uint32_t)d.seed, k1 = (uint32_t)(d.seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  const double clean = (double)(float)w;
  const double lam = active ? F * clean + b : 0.0;
  const bool small = lam < kShPoissonSwitch;
  const double ks = sh_poisson_small(small ? lam : 0.0, c[0], small && active);   // (every lane walks the wave's loop: no divergent call)
  const double n = small ? ks : sh_poisson_large(lam, c[0], c[1]);
  return (n + sigma * box_muller24_cos(c[2], c[3]) - b) / F;
}

// float32 obs_raw and IEEE half obs of a value, rounded to nearest even from float64 (the casts of the noise-free stores)
__device__ __forceinline__ void det_store(double y, size_t i, float* __restrict__ obs_raw, uint16_t* __restrict__ obs) {
  if (obs_raw) obs_raw[i] = (float)y;
  if (obs) {
    const _Float16 hv = (_Float16)y;
    obs[i] = *reinterpret_cast<const uint16_t*>(&hv);
  }
}

}  // namespace aog
