// K13: the science camera (aog_science_integrate / aog_science_clear / aog_science_read): per-env long exposures of the science arm's
// focal plane, their Strehl and encircled energy.  Off the step() path; nothing here is launched by a reset or step.
#pragma once
#include "k_common.h"
#include "k_mft_mma.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// A frame of env e on the w x w window of the science focal grid:
//   I[v][u] = | sum_{y,x} m1[v][y] E[y][x] m2[x][u] |^2,   E = exp(2 pi i ratio u_p) on the aperture, 0 outside
// u_p = psi + Mt a in revolutions of the sensing wavelength (k_phase_mfma's contraction), ratio = lambda_wfs / lambda_sci, m1 carries
// 1 / n_ap so that a flat wavefront gives 1 at the on-axis sample (row / column w / 2).  exposure [B][w][w] float64 += I, frames [B] += 1.
// The two products are K4's (k_focal.h: split-f16 operands, fp32 sums, the pupil field formed inside pass 1); pass 2 never writes a field.
// ------------------------------------------------------------------------------------------------

// The phase grid of the science arm: k_phase_mfma<.., GRID>'s contraction and LDS transposition, with screen and mirror phase scaled by
// `ratio` BEFORE they are reduced to a revolution (the ratio is no integer: a phase reduced at the sensing wavelength has lost the whole
// revolutions the science wavelength still sees).  The scaling and the reductions run in float64 (a few operations per pixel), so the
// grid is as good as the fp32 screen and the 33-bit actuators allow.  One wave per (pixel tile, env tile); grid [env][Nyp][Nxp] floats,
// kShOutside outside the aperture (written once at upload).  mask (nullable, offset to the chunk's first env): a masked-out env's grid is
// not written (pass 1 does not read it).
template <int A_PAD>
__global__ __launch_bounds__(256) void k_science_phase(const f16x8* __restrict__ modes16, const f32x4* __restrict__ psi_tile,
                                                       const f16x8* __restrict__ act16, const f16x8* __restrict__ act_ll,
                                                       const int32_t* __restrict__ ap_yx, float* __restrict__ grid, size_t env_stride, int row_stride,
                                                       int n_ptiles, int n_etiles, int n_ap, int n_env, double ratio,
                                                       const uint8_t* __restrict__ mask) {
  constexpr int NSTEP = A_PAD / 16;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), etile = blockIdx.y;
  __shared__ float grid_lds[4 * 32 * 33];
  float* grid_tile = grid_lds + (threadIdx.x >> 6) * 32 * 33;
  if (t >= n_ptiles || etile >= n_etiles) return;
  const f16x8* ms = modes16 + ((size_t)t * NSTEP * 2) * 64 + lane;
  const f16x8* as = act16 + ((size_t)etile * NSTEP * 2) * 64 + lane;
  f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    const f16x8 mh = ms[(2 * s) * 64], ml = ms[(2 * s + 1) * 64], bh = as[(2 * s) * 64], bl = as[(2 * s + 1) * 64];
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bl, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, act_ll[((size_t)etile * NSTEP + s) * 64 + lane], d, 0, 0, 0);   // (the actuators to 33 bits: see k_phase_mfma)
  }
  const size_t base = (((size_t)etile * n_ptiles + t) * 4) * 64 + lane;
  const int h = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 p = psi_tile[base + g * 64];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = 8 * g + 4 * h + r;
      // each part scaled, then reduced to a revolution, before they are added (k_phase_mfma: the sum then rounds at 2^-25 of a revolution)
      const double ps = (double)p[r] * ratio, dm = (double)(d[4 * g + r] * kPhaseUnscale) * ratio;
      const double w = (ps - rint(ps)) + (dm - rint(dm));
      grid_tile[(lane & 31) * 33 + q] = (float)(w - rint(w));
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the tile is private to the wave
  __builtin_amdgcn_wave_barrier();
  // lanes along the PIXELS of an env: 128 contiguous bytes per env wherever the aperture's rows allow
  const int qs = lane & 31, pix = t * 32 + qs;
  if (pix < n_ap) {
    const int yx = ap_yx[pix];
    const size_t at = (size_t)(yx >> 16) * row_stride + (yx & 0xffff);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int el = 2 * j + (lane >> 5), env = etile * 32 + el;
      if (env < n_env && (!mask || mask[env])) grid[(size_t)env * env_stride + at] = grid_tile[el * 33 + qs];
    }
  }
}

// The two passes are mft_pass1 / mft_pass2 (k_mft_mma.h), K4's loops, in their runtime MftWindow geometry: the output side is padded to whole
// 32-column blocks only (nvb = ceil(w / 32)), and windows of at most two blocks run the `split` form.  mask (nullable) is indexed by the
// handle's env = env0 + blockIdx.z; a masked-out env's workgroups leave before any load of its data.
// pass 1.  grid (Nxp / 128, ceil(nvb / 4), envs of the chunk); phase [env][Nyp][Nxp]; m1s [nvb][Nyp / 16] tiles; T16 [env][Nxp / 32][nvb][2] tiles
__global__ __launch_bounds__(256, 2) void k_science_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp,
                                                          int Nyp, int nvb, const uint8_t* __restrict__ mask, int env0, int split) {
  const int env = blockIdx.z;
  if (mask && !mask[env0 + env]) return;   // (workgroup-uniform)
  mft_pass1(phase, m1s, T16, Nxp, Nyp, MftWindow{nvb, split});
}
// pass 2 never writes a field: the tail squares the accumulators and adds them to the exposure.  One thread owns one pixel of one env (no
// atomics; frames add in stream order).  grid (ceil(nvb / 4) [u], ceil(nvb / 4) [v], envs of the chunk)
__global__ __launch_bounds__(256, 2) void k_science_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, double* __restrict__ exposure,
                                                          int32_t* __restrict__ frames, int Nxp, int nvb, int w, float unscale,
                                                          const uint8_t* __restrict__ mask, int env0, int split) {
  const int env = blockIdx.z;
  if (mask && !mask[env0 + env]) return;
  const double us = (double)unscale;
  mft_pass2(T16, m2s, Nxp, w, MftWindow{nvb, split}, [=](int, int u, int v, float fr, float fi) {
    const double re = (double)fr * us, im = (double)fi * us;   // (exact: unscale is a power of two)
    double* __restrict__ ex = exposure + (size_t)(env0 + env) * w * w;
    ex[(size_t)v * w + u] += fma(re, re, im * im);
  });
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) frames[env0 + env] += 1;
}

// zero the exposure and frame count of the selected envs.  grid (blocks over w^2, B)
__global__ void k_science_clear(double* __restrict__ exposure, int32_t* __restrict__ frames, const uint8_t* __restrict__ mask, int w2) {
  const int env = blockIdx.y;
  if (mask && !mask[env]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) frames[env] = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w2; i += gridDim.x * blockDim.x) exposure[(size_t)env * w2 + i] = 0.0;
}

// ---- float64 validation handles: per env, E at the science wavelength and two plain complex products (K4's k_focal_field with the uploaded
// ratio and k_cgemm_small, through focal.hip's launchers), then |F|^2 into the exposure ----
__global__ void k_science_accum64(const double2* __restrict__ F, double* __restrict__ exposure, int32_t* __restrict__ frames, int w2, int env,
                                  const uint8_t* __restrict__ mask) {
  if (mask && !mask[env]) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0) frames[env] += 1;
  if (idx >= w2) return;
  const double2 f = F[idx];
  exposure[(size_t)env * w2 + idx] += fma(f.x, f.x, f.y * f.y);
}

// ---- exposures -> mean PSF, long-exposure Strehl, encircled energy.  One workgroup (256 threads) per env of [first, first + count) ----
// bin [w^2] int32: the radial bin of each pixel of the window (-1: outside every radius); EE_k = peak_fraction x (sum over bins <= k) / frames.
// Every bin is summed in a fixed order (thread i takes pixels i, i + 256, ..., then a tree over the threads), in float64, nothing
// contracted: a result depends on the env's exposure alone.  An env with no frames reads as zeros.
struct ScienceFinishArgs {
  const double* exposure;
  const int32_t* frames;
  const int32_t* bin;
  double* psf;       // [count][w][w]   (each output nullable)
  double* strehl;    // [count]
  double* ee;        // [count][n_ee]
  int32_t* frames_out;
  int first, w, n_ee;
  double peak_fraction;
};
__global__ __launch_bounds__(256) void k_science_finish(ScienceFinishArgs p) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int j = blockIdx.x, env = p.first + j, w2 = p.w * p.w, tid = threadIdx.x;
  const double* __restrict__ ex = p.exposure + (size_t)env * w2;
  const int n = p.frames[env];
  const double fr = (double)n;
  if (p.frames_out && tid == 0) p.frames_out[j] = n;
  if (p.strehl && tid == 0) p.strehl[j] = n ? ex[(size_t)(p.w / 2) * p.w + p.w / 2] / fr : 0.0;
  if (p.psf)
    for (int i = tid; i < w2; i += 256) p.psf[(size_t)j * w2 + i] = n ? ex[i] / fr : 0.0;
  if (!p.ee) return;
  double cum = 0.0;
  for (int k = 0; k < p.n_ee; ++k) {
    double s = 0.0;
    for (int i = tid; i < w2; i += 256)
      if (p.bin[i] == k) s += ex[i];
    red[tid] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if (tid < half) red[tid] += red[tid + half];
      __syncthreads();
    }
    cum += red[0];
    if (tid == 0) p.ee[(size_t)j * p.n_ee + k] = n ? p.peak_fraction * (cum / fr) : 0.0;
    __syncthreads();   // (red is rewritten by the next bin)
  }
}

}  // namespace aog
