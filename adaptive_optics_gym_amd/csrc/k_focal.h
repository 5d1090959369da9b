// K4: focal-plane field export (single env float64 form and the batched split-f16 matrix-core form).
// The batched form's two loops are defined once, in k_mft_mma.h (mft_pass1 / mft_pass2), for K4 and the science camera; this file keeps the
// layout description and K4's kernels.  The float64 kernels at both ends serve the validation forms of K4, K11 and the science camera.
#pragma once
#include "k_common.h"
#include "k_mft_mma.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// K4  focal-plane field of one env (propagator_fiber, AO_env.py:138), off the step() path.
//   E[y][x]  = exp(2 pi i (psi + M a))  on the aperture (amplitude folded into focal_m1), 0 outside
//   T[v][x]  = sum_y m1[v][y] E[y][x];     F[v][u] = sum_x T[v][x] m2[x][u]        (float64 accumulation)
// The float64 branch is also the E of K11's and the science camera's validation handles: `ratio` scales the phase before it is reduced
// to a revolution (lambda_wfs / lambda_sci for the camera; 1.0 elsewhere, which is exact), mask (nullable): a masked-out env writes nothing.
// ------------------------------------------------------------------------------------------------
__global__ void k_focal_field(const float* __restrict__ psi_tile, const double* __restrict__ psi64, const float* __restrict__ modes_f32,
                              const double* __restrict__ modes64, const float* __restrict__ act_rev, const double* __restrict__ act_dm,
                              const int32_t* __restrict__ ap_index, double2* __restrict__ E, int env, int n_ap, int n_ptiles, int A,
                              int A_pad, int Bp, double lambda_wfs, double ratio, const uint8_t* __restrict__ mask) {
  if (mask && !mask[env]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_ap) return;
  double frac;   // the phase in revolutions, reduced to [-1/2, 1/2]
  if (psi64) {  // float64 validation handle
    double surf = 0;
    for (int k = 0; k < A; ++k) surf = fma(modes64[(size_t)p * A + k], act_dm[(size_t)env * A + k], surf);
    const double rev = (psi64[(size_t)env * n_ap + p] + 4.0 * M_PI * surf) / (2.0 * M_PI * lambda_wfs);
    frac = fma(rev, ratio, -rint(rev * ratio));   // (the scaled phase is rounded once, inside the reduction; ratio = 1: rev - rint(rev) exactly)
  } else {
    double acc = (double)psi_tile[psi_tile_index(env, p, n_ptiles)];
    const double two_over_lambda = 2.0 / lambda_wfs;   // actuators (metres) -> revolutions per unit mode, as the prologue does
    for (int k = 0; k < A; ++k) acc = fma((double)modes_f32[(size_t)p * A_pad + k], act_dm[(size_t)env * A + k] * two_over_lambda, acc);
    frac = acc - rint(acc);
  }
  double sn, cs;
  sincospi(2.0 * frac, &sn, &cs);
  E[ap_index[p]] = make_double2(cs, sn);
}

// K4, batched (aog_focal_images): both products on the f16 matrix cores with every operand split hi + lo (the step kernel's
// contraction: 3 x v_mfma_f32_32x32x16_f16 per real product, 22 significant bits per factor, exact products, fp32 sums).  The fp32
// matrix instruction this path used in round 2 runs at 1/16 of the f16 rate and does not co-execute with vector work.
//   pass 1  (k_focal_pass1):  T'^T[x][v] = sum_y E[y][x] m1'[v][y],  E = e^{2 pi i w} formed from the dense phase grid k_phase_mfma<GRID>
//           writes (one float per pixel, kShOutside outside the aperture -> E = 0) while it is loaded: E never exists in memory
//   pass 2  (k_focal_pass2):  F[v][u] = sum_x T'[v][x] m2'[x][u] / scale
// m1' = m1 2^e1, m2' = m2 2^e2 (largest component in [1/2, 1): the f16 halves stay normal), scale = 2^(e1 + e2).
// Operand tiles are stored MFMA-ready: one tile = [part: re hi, re lo, im hi, im lo][lane 64][8 f16] = 4 KiB; lane l carries row / column
// l & 31 and the 8 k-slots of k-group l >> 5.  Pass 1 leaves T' already split, in tiles [x tile of 32][v block][s][part][lane]: the 16
// accumulator registers of a lane (column v = l & 31, rows x = (r & 3) + 8 (r >> 2) + 4 (l >> 5)) are two k-groups of 8 (s = r >> 3) for
// pass 2, whose m2' table is laid out in the same order of x — the matrix instruction sums over k whatever order the slots are in, so no
// transposition happens anywhere.  Workgroup = 4 waves = 4 x 32 columns (v blocks / u blocks) of ONE 128-row span; per k-step the four
// waves produce the span's four A tiles into LDS (pass 1: one x tile each — 8 loads, 16 transcendentals, mask split; pass 2: one copied
// T' tile each), every wave then runs 4 tiles x 12 matrix instructions against its own B tile from the L2-resident table.
// The two loops are mft_pass1 / mft_pass2 (k_mft_mma.h) in their compile-time MftFull geometry: nfp is a multiple of 128, every wave's block exists.
// pass 1.  grid (Nxp / 128, nfp / 128, envs); phase [env][Nyp][Nxp]; m1s [nfp / 32][Nyp / 16] tiles; T16 [env][Nxp / 32][nfp / 32][2] tiles
__global__ __launch_bounds__(256, 2) void k_focal_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp,
                                                        int Nyp, int nfp) {
  mft_pass1(phase, m1s, T16, Nxp, Nyp, MftFull{nfp / 32});
}
// pass 2.  grid (nfp / 128 [u], nfp / 128 [v], envs); m2s [nfp / 32][Nxp / 32][2] tiles; F [env][nf][nf] complex64
__global__ __launch_bounds__(256, 2) void k_focal_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, float2* __restrict__ F, int Nxp, int nfp,
                                                        int nf, float unscale) {
  mft_pass2(T16, m2s, Nxp, nf, MftFull{nfp / 32}, [=](int env, int u, int v, float re, float im) {
    float2* Fe = F + (size_t)env * nf * nf;
    Fe[(size_t)v * nf + u] = make_float2(re * unscale, im * unscale);
  });
}

// out[r][c] = sum_k a[r][k] * b[k][c]  (complex, row-major), one thread per output; nothing for an env the mask (nullable) leaves out
__global__ void k_cgemm_small(const double2* __restrict__ a, const double2* __restrict__ b, double2* __restrict__ out, float2* __restrict__ out32,
                              int R, int K, int Cn, const uint8_t* __restrict__ mask, int env) {
  if (mask && !mask[env]) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= R * Cn) return;
  const int r = idx / Cn, c = idx - r * Cn;
  double re = 0, im = 0;
  for (int k = 0; k < K; ++k) {
    const double2 x = a[(size_t)r * K + k], y = b[(size_t)k * Cn + c];
    re = fma(x.x, y.x, fma(-x.y, y.y, re));
    im = fma(x.x, y.y, fma(x.y, y.x, im));
  }
  if (out) out[idx] = make_double2(re, im);
  if (out32) out32[idx] = make_float2((float)re, (float)im);
}

}  // namespace aog
