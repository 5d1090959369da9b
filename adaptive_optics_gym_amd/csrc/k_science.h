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

// pass 1: k_focal_pass1's loop on the window's geometry.  The output side is padded to whole 32-column v blocks only (nvb = ceil(w / 32)):
// a wave whose v block lies past the window still produces its x tile of every k-step (the four waves share that work) but issues no
// matrix instruction and stores nothing.  grid (Nxp / 128, ceil(nvb / 4), envs of the chunk); phase [env][Nyp][Nxp]; m1s [nvb][Nyp / 16]
// tiles; T16 [env][Nxp / 32][nvb][2] tiles.  mask (nullable) is indexed by the handle's env = env0 + blockIdx.z.
// split (windows of at most two blocks, nvb <= 2): the four waves share the two blocks instead — wave takes block wave & 1 against x tiles
// 2 (wave >> 1), + 1 of the span — so every wave issues matrix instructions.  Each (x tile, block) product is the same instruction sequence
// in either form: the bits do not depend on it.
__global__ __launch_bounds__(256, 2) void k_science_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp,
                                                          int Nyp, int nvb, const uint8_t* __restrict__ mask, int env0, int split) {
  __shared__ f16x8 a_lds[2][4 * kFocalTile];
  const int env = blockIdx.z;
  if (mask && !mask[env0 + env]) return;   // (workgroup-uniform, before any load of the env's data)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = blockIdx.x * 128, vb = split ? (wave & 1) : blockIdx.y * 4 + wave;
  const int t0 = split ? 2 * (wave >> 1) : 0, t1 = split ? t0 + 2 : 4;   // x tiles of the span this wave multiplies
  const bool live = vb < nvb;   // (wave-uniform)
  const int nk = Nyp / 16;
  const float* __restrict__ src = phase + ((size_t)env * Nyp + 8 * (lane >> 5)) * Nxp + x0 + 32 * wave + (lane & 31);
  const f16x8* __restrict__ bsrc = m1s + (size_t)min(vb, nvb - 1) * nk * kFocalTile + lane;
  f32x16 cr[4], ci[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { cr[t][r] = 0.f; ci[t][r] = 0.f; }
  float w[8];
  f16x8 b[4], bn[4];
  auto load_w = [&](int ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = src[(size_t)(ks * 16 + j) * Nxp];
  };
  auto load_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = bsrc[(size_t)ks * kFocalTile + q * 64];
  };
  auto produce = [&](int buf) {
    float c[8], s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = w[j] < 1.5f;
      c[j] = in ? __builtin_amdgcn_cosf(w[j]) : 0.f;
      s[j] = in ? __builtin_amdgcn_sinf(w[j]) : 0.f;
    }
    f16x8 ch, cl, sh, sl;
    split8(c, ch, cl);
    split8(s, sh, sl);
    f16x8* dst = a_lds[buf] + wave * kFocalTile + lane;
    dst[0] = ch; dst[64] = cl; dst[128] = sh; dst[192] = sl;
  };
  load_w(0);
  load_b(0, b);
  produce(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int nxt = min(ks + 1, nk - 1);
    load_w(nxt);   // (ahead of the matrix instructions, and the produce unconditional: see k_focal_pass1)
    load_b(nxt, bn);
    __builtin_amdgcn_sched_barrier(0);
    if (live) {
      const f16x8 nbh = neg8(b[2]), nbl = neg8(b[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t >= t0 && t < t1) focal_mma_tile(a_lds[ks & 1] + t * kFocalTile, lane, b, nbh, nbl, cr[t], ci[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    produce((ks + 1) & 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bn[q];
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < t0 || t >= t1) continue;
    const int xt = (x0 >> 5) + t;
    f16x8* dst = T16 + ((((size_t)env * (Nxp / 32) + xt) * nvb + vb) * 2) * kFocalTile + lane;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float vr[8], vi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { vr[j] = cr[t][8 * s2 + j]; vi[j] = ci[t][8 * s2 + j]; }
      f16x8 rh, rl, ih, il;
      split8(vr, rh, rl);
      split8(vi, ih, il);
      f16x8* dd = dst + (size_t)s2 * kFocalTile;
      dd[0] = rh; dd[64] = rl; dd[128] = ih; dd[192] = il;
    }
  }
}

// pass 2: k_focal_pass2's loop; the tail squares the accumulators and adds them to the exposure.  One thread owns one pixel of one env
// (no atomics; frames add in stream order).  grid (ceil(nvb / 4) [u], ceil(nvb / 4) [v], envs of the chunk); a workgroup multiplies the
// nt = min(4, nvb - vb0) v blocks the window has, a wave whose u block lies past the window issues no matrix instruction.
// split (nvb <= 2): wave takes u block wave & 1 against v block wave >> 1 alone, so all four waves multiply.
// (fp32 sums over x, as K4: see k_focal_pass2 for what folding them into float64 costs.)
__global__ __launch_bounds__(256, 2) void k_science_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, double* __restrict__ exposure,
                                                          int32_t* __restrict__ frames, int Nxp, int nvb, int w, float unscale,
                                                          const uint8_t* __restrict__ mask, int env0, int split) {
  __shared__ f16x8 a_lds[2][4 * kFocalTile];
  const int env = blockIdx.z;
  if (mask && !mask[env0 + env]) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ub = split ? (wave & 1) : blockIdx.x * 4 + wave, vb0 = blockIdx.y * 4;
  const int nt = min(4, nvb - vb0), nk = (Nxp / 32) * 2;
  const int t0 = split ? (wave >> 1) : 0, t1 = split ? t0 + 1 : 4;   // v blocks of the span this wave multiplies
  const bool live = ub < nvb, feeds = wave < nt;   // (wave-uniform) this wave multiplies / copies the tile of v block vb0 + wave
  const f16x8* __restrict__ asrc = T16 + ((size_t)env * (Nxp / 32) * nvb + vb0 + min(wave, nt - 1)) * 2 * kFocalTile + lane;
  const f16x8* __restrict__ bsrc = m2s + (size_t)min(ub, nvb - 1) * nk * kFocalTile + lane;
  f32x16 cr[4], ci[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { cr[t][r] = 0.f; ci[t][r] = 0.f; }
  f16x8 a[4], b[4], bn[4];
  auto load_a = [&](int ks) {
    const f16x8* p = asrc + ((size_t)(ks >> 1) * nvb * 2 + (ks & 1)) * kFocalTile;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = p[q * 64];
  };
  auto load_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = bsrc[(size_t)ks * kFocalTile + q * 64];
  };
  auto produce = [&](int buf) {
    if (!feeds) return;
    f16x8* dst = a_lds[buf] + wave * kFocalTile + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q * 64] = a[q];
  };
  load_a(0);
  load_b(0, b);
  produce(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int nxt = min(ks + 1, nk - 1);
    load_a(nxt);
    load_b(nxt, bn);
    __builtin_amdgcn_sched_barrier(0);
    if (live) {
      const f16x8 nbh = neg8(b[2]), nbl = neg8(b[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt && t >= t0 && t < t1) focal_mma_tile(a_lds[ks & 1] + t * kFocalTile, lane, b, nbh, nbl, cr[t], ci[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    produce((ks + 1) & 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bn[q];
    __syncthreads();
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) frames[env0 + env] += 1;
  const int u = ub * 32 + (lane & 31);
  if (!live || u >= w) return;
  double* __restrict__ ex = exposure + (size_t)(env0 + env) * w * w;
  const double us = (double)unscale;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < nt && t >= t0 && t < t1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = (vb0 + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (v < w) {
          const double re = (double)cr[t][r] * us, im = (double)ci[t][r] * us;   // (exact: unscale is a power of two)
          ex[(size_t)v * w + u] += fma(re, re, im * im);
        }
      }
    }
}

// zero the exposure and frame count of the selected envs.  grid (blocks over w^2, B)
__global__ void k_science_clear(double* __restrict__ exposure, int32_t* __restrict__ frames, const uint8_t* __restrict__ mask, int w2) {
  const int env = blockIdx.y;
  if (mask && !mask[env]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) frames[env] = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w2; i += gridDim.x * blockDim.x) exposure[(size_t)env * w2 + i] = 0.0;
}

// ---- float64 validation handles: per env, E at the science wavelength, two plain complex products, |F|^2 into the exposure ----
// E[y][x] = exp(2 pi i ratio u_p), u_p = (psi + 4 pi M a) / (2 pi lambda_wfs) revolutions of the sensing wavelength, on the aperture
// (k_focal_field's float64 branch with the uploaded ratio; the rest of E stays 0)
__global__ void k_science_field64(const double* __restrict__ psi64, const double* __restrict__ modes64, const double* __restrict__ act_dm,
                                  const int32_t* __restrict__ ap_index, double2* __restrict__ E, int env, int n_ap, int A, double lambda_wfs,
                                  double ratio,
                                  const uint8_t* __restrict__ mask) {
  if (mask && !mask[env]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_ap) return;
  double surf = 0;
  for (int k = 0; k < A; ++k) surf = fma(modes64[(size_t)p * A + k], act_dm[(size_t)env * A + k], surf);
  const double rev = (psi64[(size_t)env * n_ap + p] + 4.0 * M_PI * surf) / (2.0 * M_PI * lambda_wfs) * ratio;
  double sn, cs;
  sincospi(2.0 * (rev - rint(rev)), &sn, &cs);
  E[ap_index[p]] = make_double2(cs, sn);
}
// out[r][c] = sum_k a[r][k] * b[k][c]  (complex, row-major), one thread per output (k_cgemm_small's form)
__global__ void k_science_cgemm64(const double2* __restrict__ a, const double2* __restrict__ b, double2* __restrict__ out, int R, int K, int Cn,
                                  int env, const uint8_t* __restrict__ mask) {
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
  out[idx] = make_double2(re, im);
}
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
