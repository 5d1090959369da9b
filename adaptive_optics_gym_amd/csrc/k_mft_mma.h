// The split-f16 complex matrix-core product shared by the Fraunhofer transforms (K4 / K11 in k_focal.h and k_obs.h, the science camera in
// k_science.h): operand tile size, the hi + lo split and one k-step of a wave.  Layouts: see k_focal.h.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kFocalTile = 4 * 64;   // f16x8 per operand tile
// hi = x rounded to nearest f16, lo = x - hi rounded to nearest: an unbiased 22-bit operand.  (The step kernel's cheaper split by mask
// truncates both halves; here the truncation error — a fixed non-linear function of cos / sin of the phase — showed up as ghost terms of
// 1e-7 of the peak amplitude, the whole error budget of a pixel 30 dB down; this path has the vector slots to round properly.)
__device__ __forceinline__ void split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 h = (_Float16)x[j];
    hi[j] = h;
    lo[j] = (_Float16)(x[j] - (float)h);
  }
}
__device__ __forceinline__ f16x8 neg8(f16x8 v) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(f16x8, __builtin_bit_cast(u32x4, v) ^ 0x80008000u);
}
// one A tile (LDS, [part][lane]) against a wave's B tile (registers; nbh, nbl = -Bi): Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br
__device__ __forceinline__ void focal_mma_tile(const f16x8* __restrict__ a_tile, int lane, const f16x8 (&b)[4], f16x8 nbh, f16x8 nbl, f32x16& cr, f32x16& ci) {
  const f16x8 arh = a_tile[0 * 64 + lane], arl = a_tile[1 * 64 + lane], aih = a_tile[2 * 64 + lane], ail = a_tile[3 * 64 + lane];
  // (the two accumulation chains alternate; small terms first)
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[1], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[3], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, b[0], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, nbl, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, b[1], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, b[0], ci, 0, 0, 0);
}
// one k-step of a wave: its four A tiles (LDS, [tile][part][lane]) against its B tile
__device__ __forceinline__ void focal_mma(const f16x8* __restrict__ a_lds, int lane, const f16x8 (&b)[4], f32x16 (&cr)[4], f32x16 (&ci)[4]) {
  const f16x8 nbh = neg8(b[2]), nbl = neg8(b[3]);
#pragma unroll
  for (int t = 0; t < 4; ++t) focal_mma_tile(a_lds + t * kFocalTile, lane, b, nbh, nbl, cr[t], ci[t]);
}

}  // namespace aog
