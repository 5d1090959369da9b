// The two back products of one (env, quadrant) of the pyramid sensor, for k_pyr_back (k_pyramid.h) and for the gradient's k_pyr_grad_back
// (k_pyramid_grad.h), which re-forms G with the same instructions: one definition.  Layouts and the register-order argument: k_pyramid.h.
#pragma once
#include "k_common.h"
#include "k_mft_mma.h"

namespace aog {

// gr / gi [yb][xb]: the accumulators of G[y'][x'] (column x' = 32 xb + (lane & 31), rows y' = 32 yb + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), still
// at the operand scales.  kv0 .. kv1 / ku0 .. ku1: the 16-row k-steps of the quadrant's half of the window along v / u.
template <int NSB>
__device__ __forceinline__ void pyr_back_products(const f16x8* __restrict__ fop, const f16x8* __restrict__ b1s, const f16x8* __restrict__ b2s, int nvb, int env,
                                                  int sy, int sx, int kv0, int kv1, int ku0, int ku1, f32x16 (&gr)[NSB][NSB], f32x16 (&gi)[NSB][NSB]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { gr[yb][xb][r] = 0.f; gi[yb][xb][r] = 0.f; }
  for (int ub = ku0 >> 1; ub < (ku1 + 1) >> 1; ++ub) {
    f32x16 xr[NSB], xi[NSB];
#pragma unroll
    for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { xr[yb][r] = 0.f; xi[yb][r] = 0.f; }
    const f16x8* __restrict__ a = fop + (((size_t)env * nvb + ub) * nvb * 2) * kFocalTile + lane;
    for (int kv = kv0; kv < kv1; ++kv) {
      const f16x8* __restrict__ at = a + (size_t)kv * kFocalTile;
      const f16x8 a0 = at[0], a1 = at[64], a2 = at[128], a3 = at[192];
#pragma unroll
      for (int yb = 0; yb < NSB; ++yb) {
        const f16x8* __restrict__ bt = b1s + (((size_t)(sy * NSB + yb) * nvb * 2) + kv) * kFocalTile + lane;
        const f16x8 b[4] = {bt[0], bt[64], bt[128], bt[192]};
        mft_cmul(a0, a1, a2, a3, b, neg8(b[2]), neg8(b[3]), xr[yb], xi[yb]);
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int ku = 2 * ub + s2;
      if (ku < ku0 || ku >= ku1) continue;   // (wave-uniform: b2s is zero there)
#pragma unroll
      for (int yb = 0; yb < NSB; ++yb) {
        float vr[8], vi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { vr[j] = xr[yb][8 * s2 + j]; vi[j] = xi[yb][8 * s2 + j]; }
        f16x8 rh, rl, ih, il;
        split8(vr, rh, rl);
        split8(vi, ih, il);
#pragma unroll
        for (int xb = 0; xb < NSB; ++xb) {
          const f16x8* __restrict__ bt = b2s + (((size_t)(sx * NSB + xb) * nvb * 2) + ku) * kFocalTile + lane;
          const f16x8 b[4] = {bt[0], bt[64], bt[128], bt[192]};
          mft_cmul(rh, rl, ih, il, b, neg8(b[2]), neg8(b[3]), gr[yb][xb], gi[yb][xb]);
        }
      }
    }
  }
}

}  // namespace aog
