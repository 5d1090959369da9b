// K14 on the separable observation route (aog_upload_gradient_obs): the gradient of the observation that K11 forms by a matrix Fourier
// transform.  Off the step() path; nothing here is launched by a reset or step.
//
// Per env, on the pupil grid: E = A o exp(i phi) (phi the sensing-arm phase of K14), F = m1 E m2 (o x o), obs_raw_vu = |F_vu|^2 and
// L += sum_vu gbar_vu |F_vu|^2:
//     W = gbar o conj(F),   H = m1' W m2' (N x N; ' = the plain transpose),   q_yx = 2 Re(i E_yx H_yx) = -2 (sin phi Re H + cos phi Im H)
// on aperture pixels; this q joins the table part's q_p in dL/da_k = (4 pi / lambda_wfs) sum_p M_pk q_p.
//   k_grad_obs_field     fast handles: k_obs_pass2's loop (one wave per env, float64 sums over the k-steps) behind k_obs_pass1 as it stands; the
//       tail writes |F|^2 into the observation slots of `values`, forms W, divides it by a power of two that brings its largest component
//       into [4, 8) (handed to k_grad_finish in float64) and stores it split into f16 hi + lo as the A operand of the next kernel.
//   k_grad_obs_q         a wave owns one (env, 32 x 32 tile of the grid).  Q = W m2' (K = u <= 32 in two 16-deep steps, mft_cmul's split-f16 recipe) comes
//       out with the lanes along x and v in the accumulator registers, which — split — is the B operand of H = m1' Q with the operand table
//       of m1' holding v in that register order (what m2s does for pass 2): no LDS, no transposition.  H then has the lanes along x and y in
//       the registers; the wave reads its tile of the phase grid, takes v_sin_f32 / v_cos_f32 and writes -(sin Re H + cos Im H) over the
//       phase, on aperture pixels only (the grid's outside and padding keep kShOutside).
//   k_grad_obs_backward<A_PAD>   the tile range, modes contraction and reduction of k_pupil_tile.h (no screens, no actuators) with q read from
//       the grid: a wave gathers the [32 envs][32 pixels] tile of a pixel tile through focal_ap_yx with the lanes along the pixels into LDS
//       (the inverse of k_phase_mfma<GRID>'s store; pad pixels and pad envs are exact zeros) and reads it back in accumulator order, splits
//       it and contracts it with the modes (grad_mtab16).  Slab [chunk][A_PAD][Bp], added by k_grad_finish in chunk order.  No atomics.
//   k_grad_obs_w64 / k_grad_obs_q64   float64 validation handles, one env at a time around k_focal_field and k_cgemm_small.
// Magnitudes: |m1'|, |m2'| < sqrt(2) (largest component in [1/2, 1)), |W| < 8 sqrt(2): |Q| < 2^10 and |H| < 2^15 for every cotangent, inside
// the f16 range before and after the split.
#pragma once
#include "k_pupil_tile.h"
#include "k_mft_mma.h"

namespace aog {

constexpr int kGradObsWExp = 2;   // the largest component of W / wscale lies in [2^2, 2^3)
constexpr int kGradObsWop = 2 * 4 * 64;   // f16x8 per env of the W operands

// One wave per env (four per workgroup), n_env envs of this round.  T16 / m2s / unscale: k_obs_pass2's.  g_obs [n_env][o^2] (nullable: the
// values alone), values [n_env][o^2 + 2] (nullable), wop [n_env][step 2][re hi, re lo, im hi, im lo][64] f16x8: lane = row v (+ 32 x the
// half of the k-step), slot j = column u = 16 s + 8 (lane >> 5) + j; wscale [n_env].  All pointers are offset to the round's first env.
__global__ __launch_bounds__(256) void k_grad_obs_field(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, int nxt, int n_env, int o, float unscale,
                                                        const double* __restrict__ g_obs, double* __restrict__ values, _Float16* __restrict__ wop,
                                                        double* __restrict__ wscale) {
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
    mft_cmul(a[0], a[1], a[2], a[3], b, neg8(b[2]), neg8(b[3]), cr, ci);
#pragma unroll
    for (int r = 0; r < 16; ++r) { dr[r] += (double)cr[r]; di[r] += (double)ci[r]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = an[q]; b[q] = bn[q]; }
  }
  // lane: column u = lane & 31; register r: row v = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int u = lane & 31, h = lane >> 5, n_obs = o * o;
  const double us = (double)unscale;
  double big = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int v = (r & 3) + 8 * (r >> 2) + 4 * h;
    const bool have = u < o && v < o;
    const double fr = dr[r] * us, fi = di[r] * us;
    if (have && values) values[(size_t)env * (n_obs + 2) + v * o + u] = fr * fr + fi * fi;
    const double g = (have && g_obs) ? g_obs[(size_t)env * n_obs + v * o + u] : 0.0;
    dr[r] = have ? g * fr : 0.0;    // W = gbar conj(F); exact zeros in the padding
    di[r] = have ? -(g * fi) : 0.0;
    big = fmax(big, fmax(fabs(dr[r]), fabs(di[r])));
  }
  if (!g_obs) return;   // (kernel argument: wave-uniform)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off, 64));
  // a power of two: the division is exact (k_grad_coef's rule)
  const double sc = (big > 0 && big < 1e300) ? exp2((double)(ilogb(big) - kGradObsWExp)) : 1.0;
  if (lane == 0) wscale[env] = sc;
  const double inv = 1.0 / sc;
  // this lane's column u is slot u & 7 of k-step u >> 4, half (u >> 3) & 1; its 16 rows are 16 lanes of that half
  _Float16* dst = wop + (size_t)env * kGradObsWop * 8;
  const int s = u >> 4, hl = (u >> 3) & 1, j = u & 7;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int v = (r & 3) + 8 * (r >> 2) + 4 * h;
    const size_t at = ((size_t)(s * 4) * 64 + (hl * 32 + v)) * 8 + j;
    _Float16 hi, lo;
    split_f16((float)(dr[r] * inv), hi, lo);
    dst[at] = hi;
    dst[at + 64 * 8] = lo;
    split_f16((float)(di[r] * inv), hi, lo);
    dst[at + 2 * 64 * 8] = hi;
    dst[at + 3 * 64 * 8] = lo;
  }
}

// One wave per (env, y tile, x tile) of 32 x 32 grid pixels, four per workgroup: wave g -> env g / (nyt nxt), then y tile, then x tile.
// grid [n_env][Nyp][Nxp]: the phases in (revolutions, kShOutside outside), q out, in place.  m2t [nxt][step 2] tiles: lane = column x, slot j =
// u = 16 s + 8 (lane >> 5) + j.  m1t [nyt][step 2] tiles: lane = row y, slot j = v = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 8 s + j.
__global__ __launch_bounds__(256) void k_grad_obs_q(float* __restrict__ grid, const f16x8* __restrict__ wop, const f16x8* __restrict__ m1t,
                                                    const f16x8* __restrict__ m2t, int Nxp, int Nyp, int n_env) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nxt = Nxp / 32, nyt = (Nyp + 31) / 32, per_env = nxt * nyt;
  const int env = g / per_env, rem = g - env * per_env, yt = rem / nxt, xt = rem - yt * nxt;
  if (env >= n_env) return;   // (wave-uniform; the kernel has no barrier)
  // the tile's phases first: their round trip runs beside the matrix work
  float* __restrict__ tile = grid + ((size_t)env * Nyp + 32 * yt) * Nxp + 32 * xt + (lane & 31);
  float w[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int y = (r & 3) + 8 * (r >> 2) + 4 * h;
    w[r] = 32 * yt + y < Nyp ? tile[(size_t)y * Nxp] : kShOutside;
  }
  f16x8 a[4], b[4];
  f32x16 qr, qi, hr, hi;
#pragma unroll
  for (int r = 0; r < 16; ++r) { qr[r] = 0.f; qi[r] = 0.f; hr[r] = 0.f; hi[r] = 0.f; }
  // Q[v][x] = sum_u W[v][u] m2[x][u]
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[q] = wop[((size_t)env * 2 + s) * kFocalTile + q * 64 + lane];
      b[q] = m2t[((size_t)xt * 2 + s) * kFocalTile + q * 64 + lane];
    }
    mft_cmul(a[0], a[1], a[2], a[3], b, neg8(b[2]), neg8(b[3]), qr, qi);
  }
  // H[y][x] = sum_v m1[v][y] Q[v][x]: registers 8 s .. 8 s + 7 of Q are the 8 k-slots of k-step s
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float vr[8], vi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { vr[j] = qr[8 * s + j]; vi[j] = qi[8 * s + j]; }
    split8(vr, b[0], b[1]);
    split8(vi, b[2], b[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = m1t[((size_t)yt * 2 + s) * kFocalTile + q * 64 + lane];
    mft_cmul(a[0], a[1], a[2], a[3], b, neg8(b[2]), neg8(b[3]), hr, hi);
  }
  // lane: column x; register r: row y = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int y = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (w[r] < 1.5f) tile[(size_t)y * Nxp] = -fmaf(__builtin_amdgcn_sinf(w[r]), hr[r], __builtin_amdgcn_cosf(w[r]) * hi[r]);
  }
}

// grid dim3(pixel chunks, env tiles of the round): k_pupil_tile.h's geometry.  qgrid [n_env][env_stride] with row stride Nxp: what
// k_grad_obs_q left; ap_yx [n_ap] iy << 16 | ix; slabs offset to the round's first env tile.
template <int A_PAD>
__global__ __launch_bounds__(256) void k_grad_obs_backward(const float* __restrict__ qgrid, const int32_t* __restrict__ ap_yx, const f16x8* __restrict__ mtab16,
                                                           double* __restrict__ slabs, size_t env_stride, int Nxp, int n_env, int n_ptiles, int n_ap,
                                                           int Bp) {
  constexpr int NBLK = pupil_blocks(A_PAD);
  __shared__ double red[A_PAD * 32];
  __shared__ float qt_lds[4 * 32 * 33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = pupil_half(), col = lane & 31;
  const int etile = blockIdx.y;
  float* qt = qt_lds + wave * 32 * 33;   // (private to the wave)
  double acc[NBLK][16];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] = 0.0;
  pupil_for_tiles(n_ptiles, [&](int t) {
    // gather: lane = pixel col of the tile, envs 2 j + h of the env tile
    const int pix = t * 32 + col;
    const bool real = pix < n_ap;
    const int yx = real ? ap_yx[pix] : 0;
    const size_t at = (size_t)(yx >> 16) * Nxp + (yx & 0xffff);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int el = 2 * j + h, env = etile * 32 + el;
      qt[el * 33 + col] = (real && env < n_env) ? qgrid[(size_t)env * env_stride + at] : 0.f;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    // back in accumulator order: lane = env col, register j = pixel pupil_acc_row(j, h)
    float q[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] = qt[col * 33 + pupil_acc_row(j, h)];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // (the tile is rewritten by the next pixel tile)
    __builtin_amdgcn_wave_barrier();
    f16x8 qh[2], ql[2];
    pupil_split16(q, 1.f, qh, ql);
    pupil_modes_mfma<NBLK>(mtab16, t, qh, ql, acc);
  });
  pupil_reduce_store<A_PAD>(red, slabs, Bp, [&](auto put) __attribute__((always_inline)) { pupil_mode_rows<A_PAD>(acc, put); });
}

// ---- float64 validation handles, one env at a time ----
// F [o^2] complex (k_cgemm_small's) -> the env's values slots and W = gbar conj(F)
__global__ void k_grad_obs_w64(const double2* __restrict__ F, int n_obs, const double* __restrict__ g_obs, double* __restrict__ values, double2* __restrict__ W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs) return;
  const double2 f = F[i];
  if (values) values[i] = f.x * f.x + f.y * f.y;
  if (g_obs) W[i] = make_double2(g_obs[i] * f.x, -(g_obs[i] * f.y));
}
// one workgroup: q_p = 2 Re(i E_p H_p) of the env's aperture pixels (E, H on the [N][N] grid), then row k of the slab = sum_p M_pk q_p
__global__ __launch_bounds__(256) void k_grad_obs_q64(const double2* __restrict__ E, const double2* __restrict__ H, const int32_t* __restrict__ ap_index,
                                                      const double* __restrict__ modes64, double* __restrict__ q, double* __restrict__ slab, int n_ap,
                                                      int A, int Bp, int env) {
  __shared__ double sm[8];
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double2 e = E[ap_index[p]], hh = H[ap_index[p]];
    q[p] = -2.0 * (e.x * hh.y + e.y * hh.x);
  }
  __syncthreads();
  pupil64_mode_rows(modes64, q, 1, slab, n_ap, A, Bp, env, sm);
}

}  // namespace aog
