// K15's gradient (aog_pyramid_gradient): the vector-Jacobian product of the pyramid sensor's clean frame and slopes with respect to the
// mirror's actuators.  Off the step() path; nothing here is launched by a reset, a step or a sensor call.
//
// Per env ("pyramid sensor: gradient"), with gbar [4][n_s][n_s] the cotangent on the frame:
//   W_{q,j} = gbar_q o conj(G_{q,j}) / n_mod
//   V_j     = the w x w window whose quadrant block q is b1_{sy}' W_{q,j} b2_{sx}'          (' = the plain transpose)
//   H_j     = m1_j' V_j m2_j'                                                               (N x N)
//   q_p     = sum_j 2 Re(i E_p H_{j,p}), j ascending, on the aperture pixels
//   dL/da_k = (4 pi / lambda_wfs) sum_p M_pk q_p                                            (k_grad_finish's factor)
// k_pyr_grad_cot turns the call's cotangents into gbar (float64, nothing contracted) and serves the clean frame and slopes from pyr_acc
// with k_pyr_finish's arithmetic and summation order: the same bits as a photon-free sensor call.
// Fast handles run the backward passes on the matrix cores (k_pyr_grad_back, k_pyr_grad_q, then k_grad_obs_backward); float64 validation
// handles one env at a time around k_focal_field and k_cgemm_small.
#pragma once
#include "k_common.h"
#include "k_pupil_tile.h"
#include "k_pyramid_back.h"

namespace aog {

struct PyrGradCotArgs {
  const double* acc;        // [B][4][n_s][n_s] sum over the modulation points (nullable: no forward sweep ran; then g_slopes, frames, slopes are null)
  const double* g_frames;   // [B][4][n_s][n_s] nullable
  const double* g_slopes;   // [B][2 n_valid]   nullable
  double* g_pix;            // [B][4][n_s][n_s] out: gbar
  double* gscale;           // [B] out: 2^ilogb(max |gbar|) of the env (1 for a zero or non-finite one): the fast backward passes work on gbar / it
  double* frames;           // nullable out
  double* slopes;           // nullable out
  const int32_t* valid;     // [n_valid]
  const uint8_t* mask;      // nullable
  int ns, n_valid, n_mod;
};
// One workgroup (256 threads) per env.  Slopes: s_x = (I1 + I3 - I0 - I2) / Ibar, s_y = (I2 + I3 - I0 - I1) / Ibar over the valid pixels,
// Ibar = the mean over them of the quadrant sum, so with D = sum_k gx_k s_x[k] + gy_k s_y[k]:
//   dL/dI_q[k] = (sx_q gx_k + sy_q gy_k) / Ibar - D / (n_valid Ibar),   sx = (-, +, -, +), sy = (-, -, +, +)
// Every sum runs in a fixed order (thread t takes items t, t + 256, ..., then a tree over the threads).
__global__ __launch_bounds__(256) void k_pyr_grad_cot(PyrGradCotArgs p) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (p.mask && !p.mask[env]) return;
  const int n2 = p.ns * p.ns, n_pix = 4 * n2;
  const double* __restrict__ ac = p.acc ? p.acc + (size_t)env * n_pix : nullptr;
  double* __restrict__ g = p.g_pix + (size_t)env * n_pix;
  const double nm = (double)p.n_mod;
  for (int i = tid; i < n_pix; i += 256) {
    g[i] = p.g_frames ? p.g_frames[(size_t)env * n_pix + i] : 0.0;
    if (p.frames) p.frames[(size_t)env * n_pix + i] = ac[i] / nm;
  }
  if (p.g_slopes || p.slopes) {   // (kernel arguments: uniform)
    double s = 0.0;
    for (int k = tid; k < p.n_valid; k += 256) {
      const int at = p.valid[k];
      s += ((ac[at] / nm + ac[n2 + at] / nm) + ac[2 * n2 + at] / nm) + ac[3 * n2 + at] / nm;
    }
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    const double ibar = red[0] / (double)p.n_valid;
    __syncthreads();   // (red is written again below)
    const double* __restrict__ gs = p.g_slopes ? p.g_slopes + (size_t)env * 2 * p.n_valid : nullptr;
    double d = 0.0;
    for (int k = tid; k < p.n_valid; k += 256) {
      const int at = p.valid[k];
      const double i0 = ac[at] / nm, i1 = ac[n2 + at] / nm, i2 = ac[2 * n2 + at] / nm, i3 = ac[3 * n2 + at] / nm;
      const double sx = ((i1 + i3) - (i0 + i2)) / ibar, sy = ((i2 + i3) - (i0 + i1)) / ibar;
      if (p.slopes) {
        p.slopes[(size_t)env * 2 * p.n_valid + k] = sx;
        p.slopes[(size_t)env * 2 * p.n_valid + p.n_valid + k] = sy;
      }
      if (gs) d += gs[k] * sx + gs[p.n_valid + k] * sy;
    }
    if (gs) {
      red[tid] = d;
      __syncthreads();
      for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
      }
      const double c = red[0] / ((double)p.n_valid * ibar);
      for (int k = tid; k < p.n_valid; k += 256) {
        const int at = p.valid[k];
        const double gx = gs[k], gy = gs[p.n_valid + k];
        g[at] += (-gx - gy) / ibar - c;
        g[n2 + at] += (gx - gy) / ibar - c;
        g[2 * n2 + at] += (gy - gx) / ibar - c;
        g[3 * n2 + at] += (gx + gy) / ibar - c;
      }
    }
  }
  // the env's largest |gbar| (a maximum: any order gives the same bits); the barrier orders the workgroup's own writes of g_pix before it
  __syncthreads();
  double big = 0.0;
  for (int i = tid; i < n_pix; i += 256) big = fmax(big, fabs(g[i]));
  red[tid] = big;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
    __syncthreads();
  }
  if (tid == 0) p.gscale[env] = (red[0] > 0.0 && red[0] < 1e300) ? exp2((double)ilogb(red[0])) : 1.0;
}

// ---- fast handles: the backward passes on the matrix cores ----
// Per chunk of envs and modulation point j, behind k_pyr_pass1 / k_pyr_pass2 (F_j in pyr_fop):
//   k_pyr_grad_back   one wave per (env, quadrant), the four quadrants of an env in one workgroup.  G_{q,j} with k_pyr_back's own instructions
//       (pyr_back_products); W = (gbar / gscale / n_mod) conj(G) in float64 (gscale: the power of two of the env's largest |gbar|), over the
//       power of two sc that brings the largest component of the env's four W into [4, 8).  W lies with the lanes along x' and the rows y' in
//       the accumulator registers, which is the A operand (row x', K = y' in register order) of Z[x'][v] = sum_y' W[y'][x'] b1[y'][v] against
//       the table of b1' packed in that order (b1t: column v, K = y'); Z, split, is the A operand (row v, K = x') of V[v][u] = sum_x' Z[x'][v]
//       b2[u][x'] against b2t the same way.  No LDS traffic but two maxima, no transposition.  Only the 32-blocks of v and u that hold the
//       quadrant's own half are formed.  V is stored split as the A operand of the next kernel (row v, K = u in natural order), the quadrant's
//       own block of the window only: the four waves fill the window, the pads of vop stay zero from the allocation on.
//   k_pyr_grad_q      k_grad_obs_q for a window of up to 64: a wave owns (env, 32 x 32 tile of the grid); Q[v][x] = sum_u V[v][u] m2[x][u]
//       over the k-steps of the window per 32-row block of v, Q split in register order is the B operand of H[y][x] = sum_v m1[v][y] Q[v][x]
//       against m1' packed in that order.  q_j = -(sin H_re + cos H_im) is stored (first point) or added (later points) into the call's fp32
//       q grid on aperture pixels; one thread owns one pixel.
//   k_pyr_grad_qnorm  one workgroup per env, behind the last point: the env's largest |q| over the aperture -> a power of two that brings it
//       into [2^9, 2^10) before k_grad_obs_backward splits the grid into f16 halves; the power of two goes to k_pyr_grad_finish.
// Scales.  Every value that is split into f16 halves is first multiplied by a power of two (exact) measured from the data, so that the
// largest component of what one matrix product reads lies in a fixed binade whatever the cotangent — dense or one-hot:
//   W     [2^2, 2^3)   over the env's four waves (LDS maximum)
//   Z     [2^7, 2^8)   per wave and block of v; taken off V's accumulators again at once
//   V     [2^7, 2^8)   over the env's four waves (LDS maximum); sc / (this power of two) -> wscale, which k_pyr_grad_q puts on q_j
//   Q     [2^7, 2^8)   per wave and block of v; taken off that block's H again before the blocks are added
//   q     [2^9, 2^10)  per env (k_pyr_grad_qnorm)
// Upper end: every table's largest component lies in [1/2, 1), so |b1'|, |b2'|, |m1'|, |m2'| < sqrt(2), and every sum runs over K <= 64 terms:
// an operand with components below 2^8 (modulus below 2^8.5) gives a product below 2^6 2^0.5 2^8.5 = 2^15 < 65504; |W| < 2^3.5 gives |Z| < 2^10.
// Lower end: a component 2^-10 of its operand's largest still has a normal lo half (2^-3 2^-11 = 2^-14): 22 bits down to 1e-3 of the peak.
constexpr int kPyrGradWExp = 2, kPyrGradOpExp = 7, kPyrGradQExp = 9;

__device__ __forceinline__ float pyr_wave_max(float m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  return m;
}
// the power of two that brings a largest component m into [2^e, 2^(e + 1)); 1 for a zero or non-finite one
__device__ __forceinline__ float pyr_pow2_to(float m, int e) { return (m > 0.f && m < 3e38f) ? ldexpf(1.f, e - ilogbf(m)) : 1.f; }
template <int N>
__device__ __forceinline__ float pyr_max_abs(const f32x16 (&a)[N], const f32x16 (&b)[N]) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fmaxf(fabsf(a[i][r]), fabsf(b[i][r])));
  return m;
}

// grid (envs of the chunk).  b1t / b2t [2][NVB][NSB][2] tiles; vop [env][NVB][2 NVB] tiles of [part 4][lane 64][8]: lane = row v (& 31) + 32 x
// (bit 3 of u), slot = u & 7, tile = u >> 4; g_pix [B][4][n_s][n_s]; wscale [envs of the chunk]
template <int NSB, int NVB>
__global__ __launch_bounds__(256) void k_pyr_grad_back(const f16x8* __restrict__ fop, const f16x8* __restrict__ b1s, const f16x8* __restrict__ b2s,
                                                       const f16x8* __restrict__ b1t, const f16x8* __restrict__ b2t, const double* __restrict__ g_pix,
                                                       const double* __restrict__ gscale, _Float16* __restrict__ vop, double* __restrict__ wscale, int ns,
                                                       int wq, int n_mod, int4 half, double us, const uint8_t* __restrict__ mask, int env0) {
  __shared__ double bigs[4];
  __shared__ float vbig[4];
  const int env = blockIdx.x;
  if (mask && !mask[env0 + env]) return;   // (workgroup-uniform)
  const int lane = threadIdx.x & 63, h = lane >> 5, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int sy = q >> 1, sx = q & 1;
  const int kv0 = sy ? half.z : half.x, kv1 = sy ? half.w : half.y, ku0 = sx ? half.z : half.x, ku1 = sx ? half.w : half.y;
  f32x16 wr[NSB][NSB], wi[NSB][NSB];
  pyr_back_products<NSB>(fop, b1s, b2s, NVB, env, sy, sx, kv0, kv1, ku0, ku1, wr, wi);
  // W = (gbar / gscale / n_mod) conj(G): its largest component over the env's four quadrants first
  const double* __restrict__ g = g_pix + ((size_t)(env0 + env) * 4 + q) * ns * ns;
  const double gdiv = gscale[env0 + env] * (double)n_mod;
  auto gbar = [&](int yb, int xb, int r) {
    const int x = xb * 32 + (lane & 31), y = yb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    return (x < ns && y < ns) ? g[(size_t)y * ns + x] / gdiv : 0.0;
  };
  double big = 0.0;
#pragma unroll
  for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double gg = fabs(gbar(yb, xb, r));
        big = fmax(big, fmax(gg * fabs((double)wr[yb][xb][r] * us), gg * fabs((double)wi[yb][xb][r] * us)));
      }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off, 64));
  if (lane == 0) bigs[q] = big;
  __syncthreads();
  big = fmax(fmax(bigs[0], bigs[1]), fmax(bigs[2], bigs[3]));
  const double sc = (big > 0.0 && big < 1e300) ? exp2((double)(ilogb(big) - kPyrGradWExp)) : 1.0;   // a power of two: the division is exact
  const double inv = 1.0 / sc;
#pragma unroll
  for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double gg = gbar(yb, xb, r) * inv;
        wr[yb][xb][r] = (float)(gg * ((double)wr[yb][xb][r] * us));
        wi[yb][xb][r] = (float)-(gg * ((double)wi[yb][xb][r] * us));
      }
  constexpr int NKU = 2 * NVB;
  // the 32-blocks that hold the quadrant's half of the window along v and along u (wave-uniform)
  const int vb_lo = (sy * wq) >> 5, vb_hi = ((sy + 1) * wq - 1) >> 5, ub_lo = (sx * wq) >> 5, ub_hi = ((sx + 1) * wq - 1) >> 5;
  f32x16 pr[NVB][NVB], pi[NVB][NVB];
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int ub = 0; ub < NVB; ++ub)
#pragma unroll
      for (int r = 0; r < 16; ++r) { pr[vb][ub][r] = 0.f; pi[vb][ub][r] = 0.f; }
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb) {
    if (vb < vb_lo || vb > vb_hi) continue;
    // Z[x'][v] = sum_y' W[y'][x'] b1[y'][v]
    f32x16 zr[NSB], zi[NSB];
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { zr[xb][r] = 0.f; zi[xb][r] = 0.f; }
#pragma unroll
    for (int yb = 0; yb < NSB; ++yb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const f16x8* __restrict__ bt = b1t + ((((size_t)(sy * NVB + vb) * NSB + yb) * 2) + s2) * kFocalTile + lane;
        const f16x8 b[4] = {bt[0], bt[64], bt[128], bt[192]};
#pragma unroll
        for (int xb = 0; xb < NSB; ++xb) {
          float vr[8], vi[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { vr[j] = wr[yb][xb][8 * s2 + j]; vi[j] = wi[yb][xb][8 * s2 + j]; }
          f16x8 rh, rl, ih, il;
          split8(vr, rh, rl);
          split8(vi, ih, il);
          mft_cmul(rh, rl, ih, il, b, neg8(b[2]), neg8(b[3]), zr[xb], zi[xb]);
        }
      }
    const float zs = pyr_pow2_to(pyr_wave_max(pyr_max_abs<NSB>(zr, zi)), kPyrGradOpExp), zinv = 1.f / zs;
    // V[v][u] = sum_x' Z[x'][v] b2[u][x']
#pragma unroll
    for (int xb = 0; xb < NSB; ++xb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float vr[8], vi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { vr[j] = zr[xb][8 * s2 + j] * zs; vi[j] = zi[xb][8 * s2 + j] * zs; }
        f16x8 rh, rl, ih, il;
        split8(vr, rh, rl);
        split8(vi, ih, il);
#pragma unroll
        for (int ub = 0; ub < NVB; ++ub) {
          if (ub < ub_lo || ub > ub_hi) continue;
          const f16x8* __restrict__ bt = b2t + ((((size_t)(sx * NVB + ub) * NSB + xb) * 2) + s2) * kFocalTile + lane;
          const f16x8 b[4] = {bt[0], bt[64], bt[128], bt[192]};
          mft_cmul(rh, rl, ih, il, b, neg8(b[2]), neg8(b[3]), pr[vb][ub], pi[vb][ub]);
        }
      }
#pragma unroll
    for (int ub = 0; ub < NVB; ++ub)
#pragma unroll
      for (int r = 0; r < 16; ++r) { pr[vb][ub][r] *= zinv; pi[vb][ub][r] *= zinv; }
  }
  // one power of two for the env's whole window
  float vm = 0.f;
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb) vm = fmaxf(vm, pyr_max_abs<NVB>(pr[vb], pi[vb]));
  vm = pyr_wave_max(vm);
  if (lane == 0) vbig[q] = vm;
  __syncthreads();
  const float vs = pyr_pow2_to(fmaxf(fmaxf(vbig[0], vbig[1]), fmaxf(vbig[2], vbig[3])), kPyrGradOpExp);
  if (threadIdx.x == 0) wscale[env] = sc / (double)vs;
  // this lane: column u, rows v; only the quadrant's own block of the window (the rest is the other waves')
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int ub = 0; ub < NVB; ++ub) {
      const int u = 32 * ub + (lane & 31);
      const bool u_in = u >= sx * wq && u < (sx + 1) * wq;
      _Float16* __restrict__ dst = vop + ((((size_t)env * NVB + vb) * NKU + (u >> 4)) * 4 * 64) * 8 + (size_t)(32 * ((u >> 3) & 1)) * 8 + (u & 7);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int vl = (r & 3) + 8 * (r >> 2) + 4 * h, v = 32 * vb + vl;
        if (!u_in || v < sy * wq || v >= (sy + 1) * wq) continue;
        _Float16 hi, lo;
        split_f16(pr[vb][ub][r] * vs, hi, lo);
        dst[(size_t)vl * 8] = hi;
        dst[(size_t)(64 + vl) * 8] = lo;
        split_f16(pi[vb][ub][r] * vs, hi, lo);
        dst[(size_t)(128 + vl) * 8] = hi;
        dst[(size_t)(192 + vl) * 8] = lo;
      }
    }
}

// One wave per (env, y tile, x tile) of 32 x 32 grid pixels, four per workgroup (k_grad_obs_q's order).  phase [n_env][Nyp][Nxp] (revolutions,
// kShOutside outside), qgrid the same shape; m1t [y tile][NVB][2] tiles and m2t [x tile][2 NVB] tiles of THIS modulation point; nku = the
// k-steps of u the window has (ceil(w / 16))
template <int NVB>
__global__ __launch_bounds__(256) void k_pyr_grad_q(const float* __restrict__ phase, float* __restrict__ qgrid, const f16x8* __restrict__ vop,
                                                    const f16x8* __restrict__ m1t, const f16x8* __restrict__ m2t, const double* __restrict__ wscale,
                                                    int Nxp, int Nyp, int n_env, int nku, int first, const uint8_t* __restrict__ mask, int env0) {
  constexpr int NKU = 2 * NVB;
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nxt = Nxp / 32, nyt = (Nyp + 31) / 32, per_env = nxt * nyt;
  const int env = g / per_env, rem = g - env * per_env, yt = rem / nxt, xt = rem - yt * nxt;
  if (env >= n_env) return;   // (wave-uniform; the kernel has no barrier)
  if (mask && !mask[env0 + env]) return;
  const size_t at = ((size_t)env * Nyp + 32 * yt) * Nxp + 32 * xt + (lane & 31);
  float w[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int y = (r & 3) + 8 * (r >> 2) + 4 * h;
    w[r] = 32 * yt + y < Nyp ? phase[at + (size_t)y * Nxp] : kShOutside;
  }
  f32x16 hr, hi;
#pragma unroll
  for (int r = 0; r < 16; ++r) { hr[r] = 0.f; hi[r] = 0.f; }
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb) {
    f32x16 qr[1], qi[1], tr, ti;
#pragma unroll
    for (int r = 0; r < 16; ++r) { qr[0][r] = 0.f; qi[0][r] = 0.f; tr[r] = 0.f; ti[r] = 0.f; }
    for (int ku = 0; ku < nku; ++ku) {
      const f16x8* __restrict__ ap = vop + (((size_t)env * NVB + vb) * NKU + ku) * kFocalTile + lane;
      const f16x8* __restrict__ bp = m2t + ((size_t)xt * NKU + ku) * kFocalTile + lane;
      const f16x8 b[4] = {bp[0], bp[64], bp[128], bp[192]};
      mft_cmul(ap[0], ap[64], ap[128], ap[192], b, neg8(b[2]), neg8(b[3]), qr[0], qi[0]);
    }
    const float qs = pyr_pow2_to(pyr_wave_max(pyr_max_abs<1>(qr, qi)), kPyrGradOpExp), qinv = 1.f / qs;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float vr[8], vi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { vr[j] = qr[0][8 * s + j] * qs; vi[j] = qi[0][8 * s + j] * qs; }
      f16x8 b[4];
      split8(vr, b[0], b[1]);
      split8(vi, b[2], b[3]);
      const f16x8* __restrict__ ap = m1t + (((size_t)yt * NVB + vb) * 2 + s) * kFocalTile + lane;
      mft_cmul(ap[0], ap[64], ap[128], ap[192], b, neg8(b[2]), neg8(b[3]), tr, ti);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { hr[r] = fmaf(tr[r], qinv, hr[r]); hi[r] = fmaf(ti[r], qinv, hi[r]); }
  }
  const float ratio = (float)wscale[env];   // a power of two: W's over V's
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int y = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (w[r] < 1.5f) {
      const float v = -fmaf(__builtin_amdgcn_sinf(w[r]), hr[r], __builtin_amdgcn_cosf(w[r]) * hi[r]) * ratio;
      float* p = qgrid + at + (size_t)y * Nxp;
      *p = first ? v : *p + v;
    }
  }
}

// grid (envs of the chunk), behind the last modulation point: the env's q grid / a power of two that brings its largest |q| over the aperture
// into [2^9, 2^10) (a maximum: any order gives the same bits); the power of two -> qscale [B]
__global__ __launch_bounds__(256) void k_pyr_grad_qnorm(float* __restrict__ qgrid, const int32_t* __restrict__ ap_yx, double* __restrict__ qscale, size_t env_stride,
                                                        int Nxp, int n_ap, const uint8_t* __restrict__ mask, int env0) {
  __shared__ float red[256];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (mask && !mask[env0 + env]) return;
  float* __restrict__ q = qgrid + (size_t)env * env_stride;
  float m = 0.f;
  for (int p = tid; p < n_ap; p += 256) m = fmaxf(m, fabsf(q[(size_t)(ap_yx[p] >> 16) * Nxp + (ap_yx[p] & 0xffff)]));
  red[tid] = m;
  __syncthreads();
  for (int hh = 128; hh > 0; hh >>= 1) {
    if (tid < hh) red[tid] = fmaxf(red[tid], red[tid + hh]);
    __syncthreads();
  }
  const float sc = pyr_pow2_to(red[0], kPyrGradQExp);
  if (tid == 0) qscale[env0 + env] = 1.0 / (double)sc;
  for (int p = tid; p < n_ap; p += 256) q[(size_t)(ap_yx[p] >> 16) * Nxp + (ap_yx[p] & 0xffff)] *= sc;
}

// ---- float64 validation handles, one env at a time ----
// in [batch = blockIdx.y][R][C] complex -> out [batch][C][R]: the transposed tables, made once
__global__ void k_pyr_grad_transpose64(const double2* __restrict__ in, double2* __restrict__ out, int R, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * C) return;
  const size_t base = (size_t)blockIdx.y * R * C;
  const int r = i / C, c = i - r * C;
  out[base + (size_t)c * R + r] = in[base + i];
}
// G [4][n_s][n_s] complex of one modulation point -> W [sy][y'][sx][x'] = gbar conj(G) / n_mod (the quadrants of one s_y side by side: one
// product with the stacked b2' serves both)
__global__ void k_pyr_grad_w64(const double2* __restrict__ G, const double* __restrict__ g_pix, double2* __restrict__ W, int ns, int n_mod, int env,
                               const uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
  if (mask && !mask[env]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x, n2 = ns * ns;
  if (i >= 4 * n2) return;
  const int q = i / n2, r = i - q * n2, y = r / ns, x = r - y * ns;
  const double gg = g_pix[(size_t)env * 4 * n2 + i] / (double)n_mod;
  const double2 gq = G[i];
  W[((size_t)((q >> 1) * ns + y) * 2 + (q & 1)) * ns + x] = make_double2(gg * gq.x, -(gg * gq.y));
}
// q_p (+)= 2 Re(i E_p H_p) on the env's aperture pixels (E, H on the [N][N] grid): the first modulation point stores, the later ones add
__global__ void k_pyr_grad_q64(const double2* __restrict__ E, const double2* __restrict__ H, const int32_t* __restrict__ ap_index, double* __restrict__ q,
                               int n_ap, int first, int env, const uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
  if (mask && !mask[env]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_ap) return;
  const double2 e = E[ap_index[p]], hh = H[ap_index[p]];
  const double v = -2.0 * (e.x * hh.y + e.y * hh.x);
  q[p] = first ? v : q[p] + v;
}
// one workgroup: row k of the slab = sum_p M_pk q_p
__global__ __launch_bounds__(256) void k_pyr_grad_modes64(const double* __restrict__ modes64, const double* __restrict__ q, double* __restrict__ slab,
                                                          int n_ap, int A, int Bp, int env, const uint8_t* __restrict__ mask) {
  __shared__ double sm[8];
  if (mask && !mask[env]) return;
  pupil64_mode_rows(modes64, q, 1, slab, n_ap, A, Bp, env, sm);
}

// ---- slabs -> grad: k_grad_finish's first half with a mask (the rows of the envs it leaves out are not touched) ----
struct PyrGradFinishArgs {
  const double* slabs;    // [n_chunks][rows][Bp]
  const double* cscale;   // [B] nullable (1): the divisor taken off the cotangent
  const double* cscale2;  // [B] nullable (1): and the one taken off the q grid
  double* grad;           // [B][A]
  const uint8_t* mask;    // nullable
  int n_chunks, rows, Bp, A;
  double factor;          // 4 pi / lambda_wfs over the operand scales
};
__global__ __launch_bounds__(256) void k_pyr_grad_finish(PyrGradFinishArgs p) {
#pragma clang fp contract(off)
  const int env = blockIdx.x;
  if (p.mask && !p.mask[env]) return;
  const size_t slab = (size_t)p.rows * p.Bp;
  for (int k = threadIdx.x; k < p.A; k += 256) {
    const double T = pupil_slab_sum(p.slabs, p.n_chunks, slab, k, p.Bp, env);
    p.grad[(size_t)env * p.A + k] = ((T * p.factor) * (p.cscale ? p.cscale[env] : 1.0)) * (p.cscale2 ? p.cscale2[env] : 1.0);
  }
}

}  // namespace aog
