// K21: the modal disturbance's generator (aog_disturbance_*): per (env, term) a static offset plus an AR(2) vibration driven by Philox normals.
#pragma once
#include "k_common.h"

namespace aog {

// State: x [B][K], x_prev [B][K] float64, then the handle's call counter c (uint64) — the checkpoint blob as it stands.
// One thread per (env, term).  Normal j in {0, 1} of (env b, term k) of the call that finds the counter at c: philox_normal(seed, global
// env id, kDistTag + (c >> 27), ((c & 2^27 - 1) << 5) | (j << 3) | k).  Word 1 of the Philox counter (philox_normal's `ext`) separates the
// stream from the extrusion normals under the same key, whose `ext` counts an env's extrusions from 0 and stays far below the tag.
//   RESET:   x_prev = sigma n0,  x = sigma (rho1 n0 + sqrt(1 - rho1 rho1) n1)
//   ADVANCE: x_new = (a1 x + a2 x_prev) + b n0,  coeff = offset + x_new;  a masked-out env keeps its state and emits offset + x
//   PEEK:    coeff = offset + x for every env
// Every product and sum is one rounded float64 operation (mul_rn / add_rn of k_common.h: never one fma); the root comes from the host with
// the parameters, where sqrt is IEEE's: a host replay from the recorded normals is bit-exact.  No thread writes the counter: k_disturbance_tick raises it in a launch of its own behind this
// one (the threads of one launch read it while no other thread of that launch may write it).
constexpr uint32_t kDistTag = 0xD1570000u;
enum { kDistAdvance = 0, kDistReset = 1, kDistPeek = 2 };
struct DisturbanceArgs {
  double* x;                          // [B][K]
  double* x_prev;                     // [B][K]
  const unsigned long long* counter;
  const double* a1;                   // [B][K] each
  const double* a2;
  const double* b;
  const double* sigma;
  const double* rho1;
  const double* root;                 // [B][K] sqrt(1 - rho1 rho1), formed by aog_disturbance_set_params on the host
  const double* offset;
  const uint8_t* mask;                // nullable [B]
  double* coeff;                      // [B][K]; unused by a reset
  double* noise;                      // nullable: [B][K] (advance) or [B][K][2] (reset)
  int B, K, env_base, mode;
  unsigned long long seed;
};

__global__ __launch_bounds__(256) void k_disturbance(DisturbanceArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.B * a.K) return;
  const int env = i / a.K, k = i - env * a.K;
  const bool on = a.mode != kDistPeek && (!a.mask || a.mask[env]);
  const double x = a.x[i];
  if (!on) {
    if (a.mode != kDistReset) a.coeff[i] = add_rn(a.offset[i], x);
    return;
  }
  const unsigned long long c = *a.counter;
  const uint32_t genv = (uint32_t)(a.env_base + env), ext = kDistTag + (uint32_t)(c >> 27);
  const uint32_t idx = ((uint32_t)(c & 0x7FFFFFFull) << 5) | (uint32_t)k;
  const double n0 = philox_normal(a.seed, genv, ext, idx);
  if (a.mode == kDistReset) {
    const double n1 = philox_normal(a.seed, genv, ext, idx | 8u);
    const double sg = a.sigma[i];
    a.x_prev[i] = mul_rn(sg, n0);
    a.x[i] = mul_rn(sg, add_rn(mul_rn(a.rho1[i], n0), mul_rn(a.root[i], n1)));
    if (a.noise) {
      a.noise[2 * i] = n0;
      a.noise[2 * i + 1] = n1;
    }
  } else {
    const double x_new = add_rn(add_rn(mul_rn(a.a1[i], x), mul_rn(a.a2[i], a.x_prev[i])), mul_rn(a.b[i], n0));
    a.x_prev[i] = x;
    a.x[i] = x_new;
    a.coeff[i] = add_rn(a.offset[i], x_new);
    if (a.noise) a.noise[i] = n0;
  }
}

__global__ void k_disturbance_tick(unsigned long long* counter) { *counter += 1; }

}  // namespace aog
