// K15: the modulated pyramid wavefront sensor (aog_pyramid_frames / aog_pyramid_slopes / aog_pyramid_update).  Off the step() path; nothing
// here is launched by a reset or step.
#pragma once
#include "k_common.h"
#include "k_mft_mma.h"
#include "k_poisson.h"
#include "k_pyramid_back.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// Per env and modulation point j ("pyramid sensor"):
//   F_j = m1_j E m2_j                  w x w focal window (w = 2 w_q), the modulation tilt folded into m1_j / m2_j
//   G_{q,j} = b1_{sy} F_j b2_{sx}      n_s x n_s pupil image of quadrant q = 2 sy + sx; b1 / b2 are zero outside their half of the window,
//                                      so both products run over whole window blocks whatever w_q is
//   acc[env][q] (+)= |G_{q,j}|^2       float64, j ascending; k_pyr_finish divides by n_mod
// The forward passes are mft_pass1 / mft_pass2 (k_mft_mma.h) in the science camera's MftWindow geometry.  Pass 2's tail stores F_j 2^6 split
// into f16 halves as the A operands of k_pyr_back: |F_j| <= 1 whatever the wavefront (m1_j m2_j carry 1 / n_ap), so ONE power of two
// serves every env — the stored values stay below 64, the first back product below 2^13, and a value 2^-20 of the peak still has a
// normal hi half.
// fop [env][u block][v block][s 2] tiles of [part 4][lane 64][8]: lane l = row u = 32 ub + (l & 31), slot j of k-step (vb, s) = v =
// 32 vb + 16 s + (j & 3) + 8 (j >> 2) + 4 (l >> 5) — the order in which pass 2's accumulator registers hold v, which is the order b1s is packed
// in: the matrix instruction sums over k whatever order the slots are in, so no transposition happens anywhere.  Pad rows and columns of
// the blocks are zeros from the allocation on (nothing ever writes them).
// ------------------------------------------------------------------------------------------------
constexpr float kPyrFieldScale = 64.f;

// grid (Nxp / 128, ceil(nvb / 4), envs of the chunk): k_science_pass1 with the sensor's tables.  A masked-out env's workgroups leave before any load.
__global__ __launch_bounds__(256, 2) void k_pyr_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp,
                                                      int Nyp, int nvb, const uint8_t* __restrict__ mask, int env0, int split) {
  if (mask && !mask[env0 + blockIdx.z]) return;   // (workgroup-uniform)
  mft_pass1(phase, m1s, T16, Nxp, Nyp, MftWindow{nvb, split});
}
// grid (ceil(nvb / 4) [u], ceil(nvb / 4) [v], envs of the chunk); scale = unscale of the tables x kPyrFieldScale (a power of two: exact)
__global__ __launch_bounds__(256, 2) void k_pyr_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, _Float16* __restrict__ fop, int Nxp,
                                                      int nvb, int w, float scale, const uint8_t* __restrict__ mask, int env0) {
  if (mask && !mask[env0 + blockIdx.z]) return;
  mft_pass2(T16, m2s, Nxp, w, MftWindow{nvb, nvb <= 2}, [=](int env, int u, int v, float fr, float fi) {
    const int o = v & 31;
    const int lane = (u & 31) + 32 * ((o >> 2) & 1), slot = (o & 3) + 4 * ((o >> 3) & 1), s = o >> 4;
    _Float16* __restrict__ t = fop + ((((((size_t)env * nvb + (u >> 5)) * nvb + (v >> 5)) * 2 + s) * 4) * 64 + lane) * 8 + slot;
    const float re = fr * scale, im = fi * scale;
    const _Float16 rh = (_Float16)re, ih = (_Float16)im;
    t[0] = rh;
    t[64 * 8] = (_Float16)(re - (float)rh);
    t[2 * 64 * 8] = ih;
    t[3 * 64 * 8] = (_Float16)(im - (float)ih);
  });
}

// The back transform of one modulation point.  Workgroup = 4 waves = the 4 quadrants of ONE env; a wave does both complex products on
// v_mfma_f32_32x32x16_f16 with split operands:
//   X[u][y'] = sum_v F[v][u] b1[y'][v]      A = the fop tile (row u, K = v), B = b1s (column y', K = v): accumulators = column y', rows u
//   G[y'][x'] = sum_u X[u][y'] b2[u][x']    A = X straight from those accumulators (row y', K = u in register order, split in registers),
//                                           B = b2s (column x', K = u in the same order): accumulators = column x', rows y'
// over the 16-row k-steps [k0, k1) of the quadrant's half of the window in each axis (`half`: k0 / k1 of the k < 0 half, then of the
// k > 0 half; the tables are zero outside, k-steps wholly outside are skipped).  One thread owns one pixel of acc: first stores, the later
// modulation points add (stream order).  NSB = ceil(n_s / 32).  grid (envs of the chunk); b1s / b2s [2][NSB][nvb][2] tiles
template <int NSB>
__global__ __launch_bounds__(256) void k_pyr_back(const f16x8* __restrict__ fop, const f16x8* __restrict__ b1s, const f16x8* __restrict__ b2s,
                                                  double* __restrict__ acc, int nvb, int ns, int4 half, double us, int first,
                                                  const uint8_t* __restrict__ mask, int env0) {
  const int env = blockIdx.x;
  if (mask && !mask[env0 + env]) return;
  const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int sy = q >> 1, sx = q & 1;
  const int kv0 = sy ? half.z : half.x, kv1 = sy ? half.w : half.y, ku0 = sx ? half.z : half.x, ku1 = sx ? half.w : half.y;
  f32x16 gr[NSB][NSB], gi[NSB][NSB];
  pyr_back_products<NSB>(fop, b1s, b2s, nvb, env, sy, sx, kv0, kv1, ku0, ku1, gr, gi);
  double* __restrict__ out = acc + ((size_t)(env0 + env) * 4 + q) * ns * ns;
#pragma unroll
  for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb) {
      const int x = xb * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int y = yb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (x < ns && y < ns) {
          const double re = (double)gr[yb][xb][r] * us, im = (double)gi[yb][xb][r] * us;   // (exact: us is a power of two)
          const double v = fma(re, re, im * im);
          double* p = out + (size_t)y * ns + x;
          *p = first ? v : *p + v;
        }
      }
    }
}

// float64 validation handles: G [4][n_s][n_s] complex of one env and modulation point -> acc
__global__ void k_pyr_accum64(const double2* __restrict__ G, double* __restrict__ acc, int n, int env, int first, const uint8_t* __restrict__ mask) {
  if (mask && !mask[env]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double2 g = G[i];
  const double v = fma(g.x, g.x, g.y * g.y);
  double* p = acc + (size_t)env * n + i;
  *p = first ? v : *p + v;
}

// The photon stream: per (global env, detector pixel i = q n_s^2 + y n_s + x, frame) ONE Philox4x32-10 call keyed by the handle's rng_seed,
// counter {i, global env, frame lo, frame hi ^ kPyrFrameXor}; word 0 = the Poisson uniform / Box-Muller radius, word 1 = its angle.
// Word 3 tells it from every other stream under the key (k_detector.h lists them).
constexpr uint32_t kPyrFrameXor = 0x9F2A31Du;

struct PyrFinishArgs {
  double* acc;             // [B][4][n_s][n_s] sum over the modulation points -> the frame, in place
  double* frames;          // [B][4][n_s][n_s] (nullable)
  double* slopes;          // [B][2 n_valid]   (nullable)
  const int32_t* valid;    // [n_valid]
  const uint8_t* mask;     // nullable
  int ns, n_valid, n_mod, env_base;
  double photons;          // 0: no noise, no random word drawn
  unsigned long long seed;
  uint32_t frame_lo, frame_hi;
};
// One workgroup (256 threads) per env, float64, nothing contracted.  Every sum runs in a fixed order (thread t takes items t, t + 256, ...,
// then a tree over the threads): a result depends on the env's own frame alone.
__global__ __launch_bounds__(256) void k_pyr_finish(PyrFinishArgs p) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (p.mask && !p.mask[env]) return;
  const int n2 = p.ns * p.ns, n_pix = 4 * n2;
  double* __restrict__ fr = p.acc + (size_t)env * n_pix;
  const double nm = (double)p.n_mod;
  for (int base = 0; base < n_pix; base += 256) {   // (uniform trip count: the small-count sampler is walked by whole waves)
    const int i = base + tid;
    const bool active = i < n_pix;
    double v = active ? fr[i] / nm : 0.0;
    if (p.photons > 0.0) {
      uint32_t c[4] = {(uint32_t)i, (uint32_t)(p.env_base + env), p.frame_lo, p.frame_hi ^ kPyrFrameXor};
      uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
#pragma unroll
      for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
      const double lam = p.photons * v;
      const bool small = lam < kShPoissonSwitch;
      const double ks = sh_poisson_small(small ? lam : 0.0, c[0], small && active);
      v = (small ? ks : sh_poisson_large(lam, c[0], c[1])) / p.photons;
    }
    if (active) {
      fr[i] = v;
      if (p.frames) p.frames[(size_t)env * n_pix + i] = v;
    }
  }
  if (!p.slopes) return;
  // a thread reads back only what it wrote itself: valid pixel k's four quadrant values live at i = q n2 + valid[k], and i mod 256 is
  // not k mod 256 — so the frame goes through the workgroup's barrier first
  __threadfence_block();
  __syncthreads();
  double s = 0.0;
  for (int k = tid; k < p.n_valid; k += 256) {
    const int at = p.valid[k];
    s += ((fr[at] + fr[n2 + at]) + fr[2 * n2 + at]) + fr[3 * n2 + at];
  }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double ibar = red[0] / (double)p.n_valid;
  double* __restrict__ out = p.slopes + (size_t)env * 2 * p.n_valid;
  for (int k = tid; k < p.n_valid; k += 256) {
    const int at = p.valid[k];
    const double i0 = fr[at], i1 = fr[n2 + at], i2 = fr[2 * n2 + at], i3 = fr[3 * n2 + at];
    out[k] = ((i1 + i3) - (i0 + i2)) / ibar;
    out[p.n_valid + k] = ((i2 + i3) - (i0 + i1)) / ibar;
  }
}

// The integrator: act_out[env][k] = act[env][k] - gain sum_i R[k][i] (s[env][i] - ref[i]), float64, i ascending, nothing contracted.
// grid (B), one thread per actuator
__global__ __launch_bounds__(256) void k_pyr_update(const double* __restrict__ act, const double* __restrict__ slopes, const double* __restrict__ recon,
                                                    const double* __restrict__ ref, double* __restrict__ act_out, int A, int n_sl, double gain) {
#pragma clang fp contract(off)
  const int env = blockIdx.x;
  const double* __restrict__ s = slopes + (size_t)env * n_sl;
  for (int k = threadIdx.x; k < A; k += 256) {
    double sum = 0.0;
    for (int i = 0; i < n_sl; ++i) sum += recon[(size_t)k * n_sl + i] * (s[i] - ref[i]);
    act_out[(size_t)env * A + k] = act[(size_t)env * A + k] - gain * sum;
  }
}

}  // namespace aog
