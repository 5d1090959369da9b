// K11: the observation of the separable route (cfg.obs_separable) — the Fraunhofer matrix Fourier transform onto the o x o grid of
// propagator_fiber_subsample (AO_env.py:385,391,139-142), o <= 32, as two small products on the f16 matrix cores:
//   pass 1  (k_obs_pass1):  T'^T[x][v] = sum_y E[y][x] m1'[v][y],  E = e^{2 pi i w} formed from the dense phase grid of k_phase_mfma<GRID>
//   pass 2  (k_obs_pass2):  F[v][u] = sum_x T'[v][x] m2'[x][u] / scale (float64 sums over the k-steps),  obs_raw = |F|^2
// The arithmetic is K4's (k_focal.h: every operand split hi + lo rounded to nearest, three v_mfma_f32_32x32x16_f16 per real product, fp32
// sums, m1' m2' scaled by powers of two), the shape is not: the whole v side is ONE 32-row block padded from o, so K4's workgroup of four
// waves sharing a 128-row span through LDS would spend 3/4 of its matrix work on padding.  Here a wave owns one (env, 32-column x tile)
// and forms its A operand in registers — no LDS, no barrier — and pass 2 is one wave per env.
#pragma once
#include "k_detector.h"
#include "k_focal.h"

namespace aog {

// one A tile held in registers (re hi, re lo, im hi, im lo) against a B tile: Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br (focal_mma_tile's order)
__device__ __forceinline__ void obs_mma(const f16x8 (&a)[4], const f16x8 (&b)[4], f32x16& cr, f32x16& ci) {
  const f16x8 nbh = neg8(b[2]), nbl = neg8(b[3]);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[1], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[3], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[3], nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[3], b[0], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2], nbl, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2], b[1], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2], nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2], b[0], ci, 0, 0, 0);
}

// pass 1.  One wave per (env, x tile of 32 columns), four per workgroup: wave g = 4 blockIdx.x + w -> env g / nxt, x tile g % nxt.
// phase [n_env][Nyp][Nxp] (kShOutside outside the aperture and in the padding); m1s [Nyp / 16] tiles (v block 0 of K4's layout);
// T16 [n_env][nxt][s 2] tiles, T' split and in pass 2's operand order (k_focal_pass1's store with one v block).
__global__ __launch_bounds__(256) void k_obs_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp,
                                                   int Nyp, int n_env) {
  const int lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nxt = Nxp / 32, env = g / nxt, xt = g - env * nxt;
  if (env >= n_env) return;   // (wave-uniform; the kernel has no barrier)
  const int nk = Nyp / 16;
  const float* __restrict__ src = phase + ((size_t)env * Nyp + 8 * (lane >> 5)) * Nxp + 32 * xt + (lane & 31);
  const f16x8* __restrict__ bsrc = m1s + lane;
  f32x16 cr, ci;
#pragma unroll
  for (int r = 0; r < 16; ++r) { cr[r] = 0.f; ci[r] = 0.f; }
  float w[8];
  f16x8 a[4], b[4], bn[4];
  auto load_w = [&](int ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = src[(size_t)(ks * 16 + j) * Nxp];
  };
  auto load_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = bsrc[(size_t)ks * kFocalTile + q * 64];
  };
  load_w(0);
  load_b(0, b);
  for (int ks = 0; ks < nk; ++ks) {
    {   // this k-step's E tile: lane = row x, slots = rows y 16 ks + 8 (lane >> 5) + j
      float c[8], s[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = w[j] < 1.5f;
        c[j] = in ? __builtin_amdgcn_cosf(w[j]) : 0.f;
        s[j] = in ? __builtin_amdgcn_sinf(w[j]) : 0.f;
      }
      split8(c, a[0], a[1]);
      split8(s, a[2], a[3]);
    }
    // the next k-step's loads go out before this one's matrix instructions (see k_focal_pass1)
    const int nxt_ks = min(ks + 1, nk - 1);
    load_w(nxt_ks);
    load_b(nxt_ks, bn);
    __builtin_amdgcn_sched_barrier(0);
    obs_mma(a, b, cr, ci);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bn[q];
  }
  f16x8* dst = T16 + ((size_t)env * nxt + xt) * 2 * kFocalTile + lane;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    float vr[8], vi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { vr[j] = cr[8 * s2 + j]; vi[j] = ci[8 * s2 + j]; }
    f16x8 rh, rl, ih, il;
    split8(vr, rh, rl);
    split8(vi, ih, il);
    f16x8* d = dst + (size_t)s2 * kFocalTile;
    d[0] = rh; d[64] = rl; d[128] = ih; d[192] = il;
  }
}

// |F|^2 of one observation pixel, written the way k_epilogue writes the table route's: float64 power (the reward reads it), float32 obs_raw,
// IEEE half obs rounded to nearest even from float64
__device__ __forceinline__ void obs_store(double w, size_t i, double* __restrict__ pw, float* __restrict__ obs_raw, uint16_t* __restrict__ obs) {
  pw[i] = w;
  if (obs_raw) obs_raw[i] = (float)w;
  if (obs) {
    const _Float16 hv = (_Float16)w;
    obs[i] = *reinterpret_cast<const uint16_t*>(&hv);
  }
}

// pass 2.  One wave per env (four per workgroup); m2s [nxt][s 2] tiles (u block 0 of K4's layout).  Outputs [n_env][o * o], row v = y frequency.
__global__ __launch_bounds__(256) void k_obs_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, int nxt, int n_env, int o, float unscale,
                                                   double* __restrict__ pw, float* __restrict__ obs_raw, uint16_t* __restrict__ obs) {
  const int lane = threadIdx.x & 63;
  const int env = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (env >= n_env) return;
  const int nk = 2 * nxt;   // k-step ks = (x tile ks >> 1, s = ks & 1): consecutive tiles in both tables
  const f16x8* __restrict__ asrc = T16 + (size_t)env * nk * kFocalTile + lane;
  const f16x8* __restrict__ bsrc = m2s + lane;
  // The sum over x runs in float64: each k-step's 16 terms go through the matrix instruction from zero and are then added to float64
  // accumulators.  (fp32 sums over all of x, as K4's pass 2 keeps them, put pixels near 1e-3 of the peak at up to 5x the 1e-5 tolerance
  // here; one tile per wave leaves the registers for it.)
  double dr[16], di[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dr[r] = 0.0; di[r] = 0.0; }
  f16x8 a[4], b[4], an[4], bn[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { a[q] = asrc[q * 64]; b[q] = bsrc[q * 64]; }
  for (int ks = 0; ks < nk; ++ks) {
    const size_t nxt_off = (size_t)min(ks + 1, nk - 1) * kFocalTile;
#pragma unroll
    for (int q = 0; q < 4; ++q) { an[q] = asrc[nxt_off + q * 64]; bn[q] = bsrc[nxt_off + q * 64]; }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 cr, ci;
#pragma unroll
    for (int r = 0; r < 16; ++r) { cr[r] = 0.f; ci[r] = 0.f; }
    obs_mma(a, b, cr, ci);
#pragma unroll
    for (int r = 0; r < 16; ++r) { dr[r] += (double)cr[r]; di[r] += (double)ci[r]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = an[q]; b[q] = bn[q]; }
  }
  // lane: column u = lane & 31; register r: row v = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int u = lane & 31, n_obs = o * o;
  if (u >= o) return;
  const double us = (double)unscale;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int v = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (v < o) {
      const double fr = dr[r] * us, fi = di[r] * us;
      obs_store(fr * fr + fi * fi, (size_t)env * n_obs + v * o + u, pw, obs_raw, obs);
    }
  }
}

// k_obs_pass2 for handles with a detector (env0 = the handle's index of env 0 of this launch): pw keeps the clean power, obs_raw / obs take the
// noisy value.  A kernel of its own, the sums above repeated (the plain kernel keeps its arguments and code: as a shared body its loads were
// scheduled differently); every lane of the wave walks the store loop, so that the sampler is called by whole waves.
__global__ __launch_bounds__(256) void k_obs_pass2_det(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, int nxt, int n_env, int o, float unscale,
                                                       double* __restrict__ pw, float* __restrict__ obs_raw, uint16_t* __restrict__ obs, DetectorArgs d,
                                                       int env0) {
  const int lane = threadIdx.x & 63;
  const int env = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (env >= n_env) return;
  const int nk = 2 * nxt;
  const f16x8* __restrict__ asrc = T16 + (size_t)env * nk * kFocalTile + lane;
  const f16x8* __restrict__ bsrc = m2s + lane;
  double dr[16], di[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dr[r] = 0.0; di[r] = 0.0; }
  f16x8 a[4], b[4], an[4], bn[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { a[q] = asrc[q * 64]; b[q] = bsrc[q * 64]; }
  for (int ks = 0; ks < nk; ++ks) {
    const size_t nxt_off = (size_t)min(ks + 1, nk - 1) * kFocalTile;
#pragma unroll
    for (int q = 0; q < 4; ++q) { an[q] = asrc[nxt_off + q * 64]; bn[q] = bsrc[nxt_off + q * 64]; }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 cr, ci;
#pragma unroll
    for (int r = 0; r < 16; ++r) { cr[r] = 0.f; ci[r] = 0.f; }
    obs_mma(a, b, cr, ci);
#pragma unroll
    for (int r = 0; r < 16; ++r) { dr[r] += (double)cr[r]; di[r] += (double)ci[r]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = an[q]; b[q] = bn[q]; }
  }
  const int u = lane & 31, n_obs = o * o;
  const double us = (double)unscale;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if ((r & 3) + 8 * (r >> 2) >= o) break;   // (wave-uniform: no lane has a row in this register or a later one)
    const int v = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const bool have = u < o && v < o, draw = have && (d.mask == nullptr || d.mask[env0 + env] != 0);
    const double fr = dr[r] * us, fi = di[r] * us;
    const double w = fr * fr + fi * fi;
    const size_t i = (size_t)env * n_obs + v * o + u;
    const double y = det_noisy_value(d, w, env0 + env, v * o + u, draw);
    if (have) pw[i] = w;
    if (draw) det_store(y, i, obs_raw, obs);
  }
}

// work-buffer initialisation: n floats of value v
__global__ void k_obs_fill(float* __restrict__ p, size_t n, float v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// float64 validation form: |F|^2 of the fields k_cgemm_small left, [n] = [B][o * o]
__global__ void k_obs_finish64(const double2* __restrict__ F, int n, double* __restrict__ pw, float* __restrict__ obs_raw, uint16_t* __restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double2 f = F[i];
  obs_store(f.x * f.x + f.y * f.y, (size_t)i, pw, obs_raw, obs);
}
// the same for handles with a detector: whole waves enter (n rounded up by the caller's grid), element i = (env i / n_obs, pixel i % n_obs)
__global__ void k_obs_finish64_det(const double2* __restrict__ F, int n, int n_obs, double* __restrict__ pw, float* __restrict__ obs_raw,
                                   uint16_t* __restrict__ obs, DetectorArgs d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool have = i < n;
  const int env = have ? i / n_obs : 0, j = have ? i - env * n_obs : 0;
  const double2 f = F[have ? i : 0];
  const double w = f.x * f.x + f.y * f.y;
  const bool draw = have && (d.mask == nullptr || d.mask[env] != 0);
  const double y = det_noisy_value(d, w, env, j, draw);
  if (have) pw[i] = w;
  if (draw) det_store(y, (size_t)i, obs_raw, obs);
}

}  // namespace aog
