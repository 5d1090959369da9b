// K10's gradient (aog_sh_gradient): the Shack-Hartmann chain backwards.
//
// Forward, per env (k_shack.h): e = amplitude exp(2 pi i u) on the aperture (u: atmosphere + mirror + micro-lens, revolutions),
// v = crop(IFFT2(FFT2(pad e) H)) un-normalised, I = scale |v|^2, per selected lenslet F = sum I', c = sum I' (x, y) / F with I' = I + 1e-10.
// Backward of L = sum g_image I + sum g_slopes slopes:
//     g_I = g_image + [g_sx (x - c_x) + g_sy (y - c_y)] / F        (pixels of a selected lenslet; g_image elsewhere)
//     g_v = scale g_I v                                            (derivative with respect to conj v)
//     g_e = crop(IFFT2(FFT2(pad g_v) conj H))                      (the adjoint of crop F^-1 diag(H) F pad is itself with conj H)
//     g_phi = 2 Im(conj(e) g_e),   dL/da_k = (4 pi / lambda_wfs) sum_p M_pk g_phi_p
// Scales.  The kernels carry w = (g_I / gscale) (sqrt(scale) v): sqrt(scale) v is the square root of a photon count, gscale the power of two
// that brings the env's largest |g_I| into [1, 2) (k_shg_cotscale), so the complex64 passes see the same magnitudes whatever the
// cotangent; q = Im(conj(e / amplitude) A' w) is what they emit, and 2 amplitude sqrt(scale) gscale goes into the last kernel's factor.
//
//   k_shg_centroids   one wave per (lenslet, env): F, c_x, c_y from the float64 image over the lenslet's pixel list in a fixed order and a
//       fixed butterfly (no atomics: the same bits however the envs are grouped) -> coef [B][n_sub][4] = g_sx / F, g_sy / F, c_x, c_y and
//       the clean slopes.
//   k_shg_cotscale    one workgroup per env: max |g_I| -> gscale.
//   separable route (the handles k_sh_rows_sep / k_sh_cols_sep serve; same RL / LW instances, same LDS planes, 256 registers at two waves
//   per SIMD):
//   k_shg_cols_back   a wave re-runs k_sh_cols_sep's transform pair on its BC columns of G1 (v is RECOMPUTED, not stored: see DESIGN.md),
//       forms w in the layout that pair ends in (layout B: lane (p, bb) holds rows p + RL k2 of column bb), runs forward, x conj(hy),
//       inverse, keeps y < N and writes g_G1 over its own block of G1 (the block is this wave's alone, read whole before it is written).
//   k_shg_rows_back   reads g_G1 as k_sh_rows_sep wrote G1 (layout A), forward, x conj(hx) (from LDS where k_sh_rows_sep keeps hx there),
//       inverse, keeps x < N, re-forms e / amplitude from the phase grid and writes q on the pupil grid's aperture pixels (fp32), from
//       where k_grad_obs_backward gathers it into the shared pupil-tile contraction.
//   generic route (hipFFT on the padded grid, complex64 or complex128): k_shg_gv, k_shg_transfer_conj, k_shg_q and k_shg_modes (float64
//   sums over the fp32 modes in a fixed order).
#pragma once
#define AOG_SH_SHARED_ONLY   // the transform blocks and templated passes of k_shack.h; its plain kernels stay shack.hip's
#include "k_shack.h"
#include "k_pupil_tile.h"

namespace aog {

struct ShGradCot {
  const double* g_image;     // [B][N*N] nullable
  const double* coef;        // [B][n_sub][4]
  const int32_t* sub_slot;   // [N*N]
  const double* x_det;       // [N]
  int N, n_sub;
};
// g_I of pixel idx = y N + x of env, xd = x_det[x], yd = x_det[y]
__device__ __forceinline__ double sh_grad_cot_px(const ShGradCot& c, size_t env, int idx, double xd, double yd) {
  double g = c.g_image ? c.g_image[env * c.N * c.N + idx] : 0.0;
  const int s = c.sub_slot[idx];
  if (s >= 0) {
    const double2* q = reinterpret_cast<const double2*>(c.coef + (env * c.n_sub + s) * 4);
    const double2 a = q[0], b = q[1];
    g += a.x * (xd - b.x) + a.y * (yd - b.y);
  }
  return g;
}

struct ShGradCentroidArgs {
  const double* image;        // [B][N*N] clean
  const int32_t* slot_start;  // [n_sub + 1]
  const int32_t* slot_pix;
  const double* x_det;
  const double* centres;      // [n_sub][2]
  const double* slopes_ref;   // [2 n_sub]
  const double* g_slopes;     // [B][2 n_sub] nullable
  double* coef;               // [B][n_sub][4]
  double* slopes_out;         // [B][2 n_sub] nullable
  const uint8_t* mask;        // nullable
  int N, n_sub;
};
// grid (n_sub, B), 64 threads
__global__ __launch_bounds__(64) void k_shg_centroids(ShGradCentroidArgs p) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const size_t env = blockIdx.y;
  if (p.mask && !p.mask[env]) return;
  const double* img = p.image + env * p.N * p.N;
  double s0 = 0.0, sx = 0.0, sy = 0.0;
  for (int i = p.slot_start[s] + lane; i < p.slot_start[s + 1]; i += 64) {
    const int pix = p.slot_pix[i], iy = pix / p.N, ix = pix - iy * p.N;
    const double w = img[pix] + 1e-10;   // estimate([wfs_image + 1e-10]) (AO_env.py:277)
    s0 += w;
    sx = fma(w, p.x_det[ix], sx);
    sy = fma(w, p.x_det[iy], sy);
  }
  for (int off = 32; off > 0; off >>= 1) {   // (both partners add the same two numbers: every lane ends with the same bits)
    s0 += __shfl_xor(s0, off, 64);
    sx += __shfl_xor(sx, off, 64);
    sy += __shfl_xor(sy, off, 64);
  }
  if (lane != 0) return;
  const double cx = sx / s0, cy = sy / s0;
  const size_t row = env * 2 * p.n_sub;
  double* c = p.coef + (env * p.n_sub + s) * 4;
  c[0] = p.g_slopes ? p.g_slopes[row + s] / s0 : 0.0;
  c[1] = p.g_slopes ? p.g_slopes[row + p.n_sub + s] / s0 : 0.0;
  c[2] = cx;
  c[3] = cy;
  if (p.slopes_out) {
    p.slopes_out[row + s] = cx - p.centres[2 * s] - p.slopes_ref[s];
    p.slopes_out[row + p.n_sub + s] = cy - p.centres[2 * s + 1] - p.slopes_ref[p.n_sub + s];
  }
}

// grid (B), 256 threads: gscale [0 .. B) = the divisor (what the last kernel multiplies back), [B .. 2 B) = its reciprocal (what the
// kernels multiply g_I by); a maximum: any order gives the same bits
__global__ __launch_bounds__(256) void k_shg_cotscale(ShGradCot c, double* __restrict__ gscale, int B, const uint8_t* __restrict__ mask) {
  __shared__ double red[256];
  const size_t env = blockIdx.x;
  const int tid = threadIdx.x;
  if (mask && !mask[env]) return;
  double m = 0.0;
  for (int idx = tid; idx < c.N * c.N; idx += 256) {
    const int y = idx / c.N, x = idx - y * c.N;
    m = fmax(m, fabs(sh_grad_cot_px(c, env, idx, c.x_det[x], c.x_det[y])));
  }
  red[tid] = m;
  __syncthreads();
  for (int hh = 128; hh > 0; hh >>= 1) {
    if (tid < hh) red[tid] = fmax(red[tid], red[tid + hh]);
    __syncthreads();
  }
  if (tid == 0) {
    const double big = red[0];
    const int ex = (big > 0.0 && big < 1e300) ? ilogb(big) : 0;
    gscale[env] = ldexp(1.0, ex);
    gscale[B + env] = ldexp(1.0, -ex);
  }
}

// the point of evaluation (metres, float64) -> the f16 hi/lo B-operand layout, as k_sh_act16 packs the sensor mirror's
__global__ void k_shg_act16(const double* __restrict__ act, _Float16* __restrict__ act16, int B, int A, int A_pad, double two_over_lambda) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * A_pad) return;
  const int env = idx / A_pad, i = idx % A_pad;
  store_act16(act16, env, i, A_pad, (i < A) ? (float)(act[(size_t)env * A + i] * two_over_lambda) : 0.f);
}

// rows of the selected envs: src [B][row] -> dst [B][row]
__global__ void k_shg_copy_rows(const double* __restrict__ src, double* __restrict__ dst, size_t row, const uint8_t* __restrict__ mask) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= row || (mask && !mask[blockIdx.y])) return;
  dst[blockIdx.y * row + i] = src[blockIdx.y * row + i];
}

// ---- separable route ----
// G1: k_sh_rows_sep's output, [B][N / BC][N][BC]; overwritten by g_G1 in the same layout.  hyq: k_sh_cols_sep's table, conjugated on load.
template <int RL, int LW>
__global__ __launch_bounds__(64 * kShFftWaves, 2) void k_shg_cols_back(float2* __restrict__ G1, const float2* __restrict__ tw, const float2* __restrict__ hyq,
                                                                       ShGradCot c, const double* __restrict__ gmul, float rs, const uint8_t* __restrict__ mask) {
  extern __shared__ float lds_shfft[];
  constexpr int L = LW * RL, N = L / 2, BC = 64 / RL, NK = N / RL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cg = blockIdx.x * kShFftWaves + wave;
  const size_t env = blockIdx.y;
  if (cg * BC >= N) return;
  if (mask && !mask[env]) return;
  const int pp = lane / BC, bb = lane - pp * BC;
  const int x = cg * BC + bb;
  float2* blk = G1 + env * N * N + (size_t)cg * N * BC + lane;   // element (y = pp + RL k2, bb) at lane + 64 k2
  cf32 v[64];
  static_for<64>([&](auto kc) {
    constexpr int k2 = decltype(kc)::v;
    if constexpr (k2 < NK) { const float2 t = blk[(size_t)k2 * 64]; v[k2] = cf32{t.x, t.y}; }
    else v[k2] = cf32{0.f, 0.f};
  });
  float* lbuf = lds_shfft + (size_t)wave * 64 * 65;
  // v again, as k_sh_cols_sep forms it
  sh_fft_b2a<RL, true, LW>(v, lbuf, tw);
  static_for<RL>([&](auto rc) {
    constexpr int r = decltype(rc)::v;
    const float2 h = hyq[r * 64 + lane];
    static_for<BC>([&](auto bc) { constexpr int i = decltype(bc)::v * RL + r; v[i] = cmul(v[i], cf32{h.x, h.y}); });
  });
  sh_fft_a2b<RL, false, LW>(v, lbuf, tw);
  // w = (g_I / gscale) (sqrt(scale) v) on rows y < N; the rows the forward pass drops carry no cotangent
  // The pixels are walked by a REAL loop with v parked in the wave's LDS plane (each lane its own NK slots, as k_sh_cols_sep's FUSED tail
  // parks its intensities): unrolled, the 32 pixels' float64 cotangents beside 128 registers of v spilled 120 - 290 registers.
  static_assert((size_t)NK * 64 * sizeof(float2) <= (size_t)64 * 65 * sizeof(float), "v of a wave fits its transform plane");
  float2* vp = reinterpret_cast<float2*>(lbuf) + lane;
  static_for<NK>([&](auto kc) { constexpr int k2 = decltype(kc)::v; vp[k2 * 64] = make_float2(v[k2].x, v[k2].y); });
  const double gm = gmul[env], xd = c.x_det[x];
#pragma unroll 2
  for (int k2 = 0; k2 < NK; ++k2) {
    const int y = pp + RL * k2;
    const float g = (float)(sh_grad_cot_px(c, env, y * N + x, xd, c.x_det[y]) * gm);
    const float2 t = vp[k2 * 64];
    vp[k2 * 64] = make_float2(g * (t.x * rs), g * (t.y * rs));
  }
  static_for<64>([&](auto kc) {
    constexpr int k2 = decltype(kc)::v;
    if constexpr (k2 < NK) { const float2 t = vp[k2 * 64]; v[k2] = cf32{t.x, t.y}; }
    else v[k2] = cf32{0.f, 0.f};
  });
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the plane is the next transform's
  __builtin_amdgcn_wave_barrier();
  sh_fft_b2a<RL, true, LW>(v, lbuf, tw);
  static_for<RL>([&](auto rc) {
    constexpr int r = decltype(rc)::v;
    const float2 h = hyq[r * 64 + lane];
    static_for<BC>([&](auto bc) { constexpr int i = decltype(bc)::v * RL + r; v[i] = cmul(v[i], cf32{h.x, -h.y}); });
  });
  sh_fft_a2b<RL, false, LW>(v, lbuf, tw);
  static_for<NK>([&](auto kc) { constexpr int k2 = decltype(kc)::v; blk[(size_t)k2 * 64] = make_float2(v[k2].x, v[k2].y); });
}

// phase: the grid k_sh_rows_sep read; gG1: k_shg_cols_back's output; qgrid [B][N][N], aperture pixels written; hxq: k_sh_rows_sep's table
template <int RL, int LW>
__global__ __launch_bounds__(64 * kShFftWaves, 2) void k_shg_rows_back(const float* __restrict__ phase, const float2* __restrict__ gG1, float* __restrict__ qgrid,
                                                                       const float2* __restrict__ tw, const float2* __restrict__ hxq,
                                                                       const uint8_t* __restrict__ mask) {
  extern __shared__ float lds_shfft[];
  constexpr int L = LW * RL, N = L / 2, BC = 64 / RL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int iy0 = (blockIdx.x * kShFftWaves + wave) * BC;
  const size_t env = blockIdx.y;
  if (mask && !mask[env]) return;   // (workgroup-uniform)
  constexpr bool HX_LDS = kShHxInLds<RL, LW>;
  cf32* hx_lds = reinterpret_cast<cf32*>(lds_shfft + (size_t)kShFftWaves * 64 * 65);
  if constexpr (HX_LDS) {
    static_for<L / (64 * kShFftWaves)>([&](auto uc) {
      const int en = (int)threadIdx.x + 64 * kShFftWaves * decltype(uc)::v;   // entry p + RL k2 lives at hxq[k2][BC p]
      const float2 t = hxq[(en / RL) * 64 + BC * (en % RL)];
      hx_lds[en] = cf32{t.x, -t.y};
    });
    __syncthreads();
  }
  if (iy0 >= N) return;
  const int la = min(lane, LW - 1);
  const float2* src = gG1 + env * N * N;
  cf32 v[64];
  static_for<64>([&](auto ic) {
    constexpr int i = decltype(ic)::v;
    constexpr int bb = i / RL, r = i % RL;
    if constexpr (r < RL / 2) {
      const int x = la + LW * r;
      const float2 t = src[((size_t)(x / BC) * N + (iy0 + bb)) * BC + (x % BC)];
      v[i] = cf32{t.x, t.y};
    } else {
      v[i] = cf32{0.f, 0.f};   // the zero padding
    }
  });
  float* lbuf = lds_shfft + (size_t)wave * 64 * 65;
  sh_fft_a2b<RL, true, LW>(v, lbuf, tw);
  if constexpr (HX_LDS) {
    const cf32* hl = hx_lds + lane / BC;
    static_for<64>([&](auto kc) { constexpr int k2 = decltype(kc)::v; v[k2] = cmul(v[k2], hl[RL * k2]); });
  } else {
    const float2* hq = hxq + lane;
    static_for<8>([&](auto gc) {   // (eight table loads at a time, as in k_sh_rows_sep)
      constexpr int g8 = decltype(gc)::v;
      float2 t8[8];
      static_for<8>([&](auto jc) { constexpr int k2 = 8 * g8 + decltype(jc)::v; if constexpr (k2 < LW) t8[decltype(jc)::v] = hq[k2 * 64]; });
      static_for<8>([&](auto jc) {
        constexpr int k2 = 8 * g8 + decltype(jc)::v;
        if constexpr (k2 < LW) v[k2] = cmul(v[k2], cf32{t8[decltype(jc)::v].x, -t8[decltype(jc)::v].y});
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  sh_fft_b2a<RL, false, LW>(v, lbuf, tw);
  if (LW == 64 || lane < LW) {
    const float* ph = phase + (env * N + iy0) * N + lane;
    float* dst = qgrid + (env * N + iy0) * N + lane;
    static_for<64>([&](auto ic) {
      constexpr int i = decltype(ic)::v;
      constexpr int bb = i / RL, r = i % RL;
      if constexpr (r < RL / 2) {
        const float u = ph[(size_t)bb * N + LW * r];
        if (u <= 1.0f) {   // an aperture pixel: q = Im(conj(e / amplitude) g_e)
          float sn, cs;
          sincospif(2.0f * u, &sn, &cs);
          dst[(size_t)bb * N + LW * r] = cs * v[i].y - sn * v[i].x;
        }
      }
    });
  }
}

// grid (B), behind k_shg_rows_back: the env's q grid x the power of two that brings its largest |q| over the aperture into [2^9, 2^10) before
// k_grad_obs_backward splits the grid into f16 halves (a maximum: any order gives the same bits); its reciprocal -> qscale [B]
__global__ __launch_bounds__(256) void k_shg_qnorm(float* __restrict__ qgrid, const int32_t* __restrict__ ap_yx, double* __restrict__ qscale, int N, int n_ap,
                                                   const uint8_t* __restrict__ mask) {
  __shared__ float red[256];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (mask && !mask[env]) return;
  float* __restrict__ q = qgrid + (size_t)env * N * N;
  float m = 0.f;
  for (int p = tid; p < n_ap; p += 256) m = fmaxf(m, fabsf(q[(size_t)(ap_yx[p] >> 16) * N + (ap_yx[p] & 0xffff)]));
  red[tid] = m;
  __syncthreads();
  for (int hh = 128; hh > 0; hh >>= 1) {
    if (tid < hh) red[tid] = fmaxf(red[tid], red[tid + hh]);
    __syncthreads();
  }
  const float big = red[0];
  const float sc = (big > 0.f && big < 3e38f) ? ldexpf(1.f, 9 - ilogbf(big)) : 1.f;
  if (tid == 0) qscale[env] = 1.0 / (double)sc;
  for (int p = tid; p < n_ap; p += 256) q[(size_t)(ap_yx[p] >> 16) * N + (ap_yx[p] & 0xffff)] *= sc;
}

// ---- generic route: hipFFT on the padded 2N x 2N grid, CT = float2 or double2 ----
// pad [B][2N][2N]: v in its first N x N corner -> w there, zeros everywhere else (the input of the backward propagation, in place)
template <typename CT>
__global__ void k_shg_gv(CT* __restrict__ pad, ShGradCot c, const double* __restrict__ gmul, double rs, const uint8_t* __restrict__ mask) {
  const int N = c.N, L = 2 * N;
  const size_t env = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= L * L || (mask && !mask[env])) return;
  const int y = idx / L, x = idx - y * L;
  CT* at = pad + env * L * L + idx;
  CT o;
  o.x = 0;
  o.y = 0;
  if (y < N && x < N) {
    using T = decltype(o.x);
    const T g = (T)(sh_grad_cot_px(c, env, y * N + x, c.x_det[x], c.x_det[y]) * gmul[env]);
    const CT a = *at;
    o.x = g * (a.x * (T)rs);
    o.y = g * (a.y * (T)rs);
  }
  *at = o;
}
template <typename CT>
__global__ void k_shg_transfer_conj(CT* __restrict__ f, const CT* __restrict__ tf, size_t per_env, const uint8_t* __restrict__ mask) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per_env || (mask && !mask[blockIdx.y])) return;
  CT* v = f + (size_t)blockIdx.y * per_env + idx;
  const CT a = *v, b = tf[idx];
  CT o;
  o.x = a.x * b.x + a.y * b.y;
  o.y = a.y * b.x - a.x * b.y;
  *v = o;
}
// q [B][n_ap] = Im(conj(e / amplitude) g_e) per packed aperture pixel, e re-formed as k_sh_field forms it
template <typename CT>
__global__ void k_shg_q(const CT* __restrict__ pad, const float* __restrict__ phase_tile, const int32_t* __restrict__ ap_index, const double2* __restrict__ mla_phase,
                        double* __restrict__ q, int n_ap, int n_ptiles, int N, const uint8_t* __restrict__ mask) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = blockIdx.y;
  if (p >= n_ap || (mask && !mask[env])) return;
  const double rev = (double)phase_tile[psi_tile_index(env, p, n_ptiles)];
  double sn, cs;
  sincospi(2.0 * (rev - rint(rev)), &sn, &cs);
  const int flat = ap_index[p];
  const int iy = flat / N, ix = flat - iy * N;
  const double2 m = mla_phase[flat];
  const double ex = cs * m.x - sn * m.y, ey = cs * m.y + sn * m.x;
  const CT g = pad[(size_t)env * 4 * N * N + (size_t)iy * 2 * N + ix];
  q[(size_t)env * n_ap + p] = ex * (double)g.y - ey * (double)g.x;
}
// grid (B), 256 threads: slab [A][Bp] row k = sum_p M_pk q_p, float64 sums in a fixed order over the handle's fp32 modes [n_ap_pad][A_pad]
__global__ __launch_bounds__(256) void k_shg_modes(const float* __restrict__ modes_f32, const double* __restrict__ q, double* __restrict__ slab, int n_ap, int A,
                                                   int A_pad, int Bp, const uint8_t* __restrict__ mask) {
  __shared__ double sm[8];
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  const double* qe = q + (size_t)env * n_ap;
  for (int k = 0; k < A; ++k) {
    double v = 0;
    for (int p = threadIdx.x; p < n_ap; p += blockDim.x) v = fma((double)modes_f32[(size_t)p * A_pad + k], qe[p], v);
    const double T = block_reduce_sum(v, sm);
    if (threadIdx.x == 0) slab[(size_t)k * Bp + env] = T;
  }
}
// slabs [n_chunks][rows][Bp] -> grad [B][A] of the selected envs: the chunks in order, x factor x the two powers of two taken off on the way
struct ShGradFinishArgs {
  const double* slabs;
  const double* gscale;   // [B]
  const double* qscale;   // [B] nullable (1)
  double* grad;
  const uint8_t* mask;    // nullable
  int n_chunks, rows, Bp, A;
  double factor;
};
__global__ __launch_bounds__(256) void k_shg_finish(ShGradFinishArgs p) {
#pragma clang fp contract(off)
  const int env = blockIdx.x;
  if (p.mask && !p.mask[env]) return;
  const size_t slab = (size_t)p.rows * p.Bp;
  for (int k = threadIdx.x; k < p.A; k += 256) {
    const double T = pupil_slab_sum(p.slabs, p.n_chunks, slab, k, p.Bp, env);
    p.grad[(size_t)env * p.A + k] = ((T * p.factor) * p.gscale[env]) * (p.qscale ? p.qscale[env] : 1.0);
  }
}
// the float64 transfer function [n] complex -> complex64 (pruned handles keep none for the padded grid)
__global__ void k_shg_tf32(const double2* __restrict__ tf, float2* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = make_float2((float)tf[i].x, (float)tf[i].y);
}

}  // namespace aog
