// K14: the analytic gradient of observation, power and Strehl with respect to the mirror (aog_upload_gradient, aog_output_gradient): the
// fused pupil pass run backwards.  Off the step() path; nothing here is launched by a reset or step.
//
// With phi_p = 2 pi u_p the sensing-arm phase, E_p = exp(i phi_p), Z_j = sum_m coef[j][m] sum_p E_p g_m(p) and L = sum_j gbar_j |Z_j|^2
// (the science arm alike with E^sci_p = exp(i r phi_p), r = lambda_wfs / lambda_sci):
//     C_m = sum_j gbar_j conj(Z_j) coef[j][m],  H_p = sum_m C_m g_m(p),  q_p = 2 Re(i E_p H_p) = -2 (cos phi_p Im H_p + sin phi_p Re H_p),
//     dL/da_k = (4 pi / lambda_wfs) sum_p M_pk q_p            (the science arm's q_p carries the extra factor r).
// The two fast kernels run on the loop, contractions and reduction of k_pupil_tile.h, which explains the register order they rely on.
//   k_grad_forward<A_PAD>   fast handles: u (pupil_phase_mfma), sin / cos at both wavelengths, and the cos / sin planes, split as they lie, are the
//       B operands of the table contraction (A = the wfs tables, <= 28 rows in one block of 32: grad_ftab16).  The one science table is
//       summed on the vector unit in float64.  fp32 accumulators are added to float64 after every tile.  Slab [chunk][66][Bp]: rows
//       m = U_m, 32 + m = V_m (scaled by the tables' operand scale), 64 / 65 = U / V of the science arm.
//   k_grad_coef             one workgroup per env, float64, nothing contracted: slabs added in chunk order, Z_j, the values, C_m; C is divided
//       by its largest component before it is split into f16 operands (its magnitude follows the cotangents and the Strehl over orders);
//       the divisor goes to k_grad_finish in float64.
//   k_grad_backward<A_PAD>  fast handles: per pixel tile H = g' C on the matrix cores (A = the tables transposed: 32 pixel rows, K = 32 tables
//       in two steps, grad_ttab16; B = Re C, Im C of the env tile, resident), q on the vector unit, q split as the B operand of the modes
//       contraction (grad_mtab16).  Pad pixels have zero table rows and pad envs zero C: both contribute exact zeros.  Slab
//       [chunk][A_PAD][Bp].  No atomics, no B x n_ap intermediate.
//   k_grad_ref_forward / k_grad_ref_backward   float64 validation handles, one workgroup per env, in the style of k_wavefront_ref.
//   k_grad_finish           one workgroup per env: slabs in chunk order, the scales, grad_act, and the action chain for grad_action.
//       On the separable observation route with aog_upload_gradient_obs a second slab set (k_gradient_obs.h: the observation's q contracted
//       with the modes) is added with scales of its own; without it the sum is the first set's alone, bit for bit.
#pragma once
#include "k_pupil_tile.h"

namespace aog {

constexpr int kGradFwdRows = 66;        // rows of a forward slab of the fast kernels
constexpr float kGradQScale = 0.0625f;  // q is scaled by 2^-4 x the tables' scale before it is split (|q| <= 2 (28 + 2) x 256: inside the f16 range)

// cos / sin of 2 pi u and of 2 pi ratio u for the lane's 16 pixels of tile t.  Pad pixels of the last tile read as cos = sin = 0 in both arms.
template <int NSTEP>
__device__ __forceinline__ void grad_tile_trig(const f16x8* __restrict__ modes16, int t, const f16x8 (&bh)[NSTEP], const f16x8 (&bl)[NSTEP],
                                               const f32x4 (&pc)[4], int n_ap, double ratio, float (&cw)[16], float (&sw)[16], float (&cs)[16],
                                               float (&ss)[16]) {
  const f32x16 d = pupil_phase_mfma<NSTEP>(modes16, t, bh, bl);
  const int left = pupil_left(n_ap, t);
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 4 * g + r;
      const float u = fmaf(d[j], kPhaseUnscale, pc[g][r]);
      const bool real = 8 * g + r < left;
      float s1, c1;
      sincos_rev<1>(u, s1, c1);
      // the science arm: scaled in float64 BEFORE the reduction to a revolution (the ratio is no integer)
      const double us = (double)u * ratio;
      const float ur = (float)(us - rint(us));
      cw[j] = real ? c1 : 0.f;
      sw[j] = real ? s1 : 0.f;
      cs[j] = real ? __builtin_amdgcn_cosf(ur) : 0.f;
      ss[j] = real ? __builtin_amdgcn_sinf(ur) : 0.f;
    }
}

template <int A_PAD>
__global__ __launch_bounds__(256) void k_grad_forward(const f16x8* __restrict__ modes16, const f16x8* __restrict__ ftab16,
                                                      const double* __restrict__ stab, const f32x4* __restrict__ psi_tile,
                                                      const f16x8* __restrict__ act16, double* __restrict__ slabs, int n_ptiles, int n_ap, int Bp,
                                                      double ratio) {
  constexpr int NSTEP = A_PAD / 16;
  __shared__ double red[kGradFwdRows * 32];
  const int lane = threadIdx.x & 63, h = pupil_half();
  double aU[16], aV[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) { aU[j] = 0.0; aV[j] = 0.0; }
  double su = 0.0, sv = 0.0;
  // (pupil_tile_loop written out: through the template this kernel's A_PAD = 64 form needs 10 more accumulator registers and loses a wave)
  const int etile = blockIdx.y;
  f16x8 bh[NSTEP], bl[NSTEP];
  {
    const f16x8* asrc = act16 + ((size_t)etile * NSTEP * 2) * 64 + lane;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) { bh[s] = asrc[(2 * s) * 64]; bl[s] = asrc[(2 * s + 1) * 64]; }
  }
  const PupilTileRange tiles = pupil_tile_range(n_ptiles);
  f32x4 pc[4], pn[4];
  auto load_psi = [&](int tile, f32x4 (&pp)[4]) {
    const size_t base = (((size_t)etile * n_ptiles + tile) * 4) * 64 + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) pp[g] = psi_tile[base + g * 64];
  };
  if (tiles.t < tiles.t_end) load_psi(tiles.t, pc);
  for (int t = tiles.t; t < tiles.t_end; t += kPupilWaves) {   // (wave-uniform)
    if (t + kPupilWaves < tiles.t_end) load_psi(t + kPupilWaves, pn);
    float cw[16], sw[16], cs[16], ss[16];
    grad_tile_trig<NSTEP>(modes16, t, bh, bl, pc, n_ap, ratio, cw, sw, cs, ss);
    f16x8 ch[2], cl[2], sh[2], sl[2];
    pupil_split16(cw, 1.f, ch, cl);
    pupil_split16(sw, 1.f, sh, sl);
    const f16x8* ts = ftab16 + ((size_t)t * 4) * 64 + lane;
    f32x16 U = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, V = U;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f16x8 th = ts[(s * 2) * 64], tl = ts[(s * 2 + 1) * 64];
      U = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ch[s], U, 0, 0, 0);
      U = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, cl[s], U, 0, 0, 0);
      U = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, ch[s], U, 0, 0, 0);
      V = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, sh[s], V, 0, 0, 0);
      V = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, sl[s], V, 0, 0, 0);
      V = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, sh[s], V, 0, 0, 0);
    }
    const double* st = stab + ((size_t)t * 2 + h) * 16;   // (the science table in accumulator order)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      aU[j] += (double)U[j];
      aV[j] += (double)V[j];
      const double g = st[j];
      su = fma((double)cs[j], g, su);
      sv = fma((double)ss[j], g, sv);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) pc[g] = pn[g];
  }
  su += __shfl_down(su, 32, 64);   // (the two half-waves hold different pixels of the same env)
  sv += __shfl_down(sv, 32, 64);
  pupil_reduce_store<kGradFwdRows>(red, slabs, Bp, [&](auto put) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      put(pupil_acc_row(j, h), aU[j]);
      put(32 + pupil_acc_row(j, h), aV[j]);
    }
    if (h != 0) return;
    put(64, su);
    put(65, sv);
  });
}

template <int A_PAD>
__global__ __launch_bounds__(256) void k_grad_backward(const f16x8* __restrict__ modes16, const f16x8* __restrict__ ttab16,
                                                       const double* __restrict__ stab, const f16x8* __restrict__ mtab16,
                                                       const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16,
                                                       const f16x8* __restrict__ cop16, const float* __restrict__ csci, double* __restrict__ slabs,
                                                       int n_ptiles, int n_ap, int Bp, double ratio, float tscale) {
  constexpr int NSTEP = A_PAD / 16, NBLK = pupil_blocks(A_PAD);
  __shared__ double red[A_PAD * 32];
  const int lane = threadIdx.x & 63, h = pupil_half(), etile = blockIdx.y;
  // Re C, Im C of this env tile (K = 32 tables in two steps, hi | lo) stay in registers
  f16x8 crh[2], crl[2], cih[2], cil[2];
  {
    const f16x8* cs16 = cop16 + ((size_t)etile * 8) * 64 + lane;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      crh[s] = cs16[(s * 4 + 0) * 64]; crl[s] = cs16[(s * 4 + 1) * 64];
      cih[s] = cs16[(s * 4 + 2) * 64]; cil[s] = cs16[(s * 4 + 3) * 64];
    }
  }
  // the science arm's one table: H = C_s g_s(p); -2 r C_s at the operand scale of q
  const int env = etile * 32 + (lane & 31);
  const float kq = -2.f * kGradQScale, ks = kq * (float)ratio * tscale;
  const float csr = csci[2 * env] * ks, csi = csci[2 * env + 1] * ks;
  double acc[NBLK][16];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] = 0.0;
  f16x8 bh[NSTEP], bl[NSTEP];
  pupil_tile_loop<NSTEP>(psi_tile, act16, n_ptiles, bh, bl, [&](int t, const f32x4 (&pc)[4]) {
    float cw[16], sw[16], cs[16], ss[16];
    grad_tile_trig<NSTEP>(modes16, t, bh, bl, pc, n_ap, ratio, cw, sw, cs, ss);
    const f16x8* ts = ttab16 + ((size_t)t * 4) * 64 + lane;
    f32x16 Hr = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, Hi = Hr;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f16x8 th = ts[(s * 2) * 64], tl = ts[(s * 2 + 1) * 64];
      Hr = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, crh[s], Hr, 0, 0, 0);
      Hr = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, crl[s], Hr, 0, 0, 0);
      Hr = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, crh[s], Hr, 0, 0, 0);
      Hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, cih[s], Hi, 0, 0, 0);
      Hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, cil[s], Hi, 0, 0, 0);
      Hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, cih[s], Hi, 0, 0, 0);
    }
    const double* st = stab + ((size_t)t * 2 + h) * 16;
    float q[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float qw = kq * fmaf(cw[j], Hi[j], sw[j] * Hr[j]);
      const float qs = (float)st[j] * fmaf(cs[j], csi, ss[j] * csr);
      q[j] = qw + qs;
    }
    f16x8 qh[2], ql[2];
    pupil_split16(q, 1.f, qh, ql);
    pupil_modes_mfma<NBLK>(mtab16, t, qh, ql, acc);
  });
  pupil_reduce_store<A_PAD>(red, slabs, Bp, [&](auto put) __attribute__((always_inline)) { pupil_mode_rows<A_PAD>(acc, put); });
}

// ---- per env: Z_j, the values the gradient is taken at, C_m ----
struct GradCoefArgs {
  const double* slabs;     // [n_chunks][rows][Bp]: U_w[m] = row m, V_w[m] = row TW + m, U_s[m] = row 2 TW + m, V_s[m] = row 2 TW + TS + m
  int n_chunks, rows, Bp, TW, TS;
  int MRW, MRS;            // tables in use per arm
  int n_obs_tab, n_out;    // observation outputs among the rows of wfs_coef (0 on the separable route), all rows of wfs_coef
  int n_obs;               // o^2: the layout of g_obs and values
  const double* wfs_coef;  // [n_out][MRW][2]
  const double* sci_coef;  // [MRS][2]
  double inv_tscale;       // the wfs sums' operand scale, inverted (1 for the float64 kernels)
  const double* g_obs;     // [B][n_obs]  nullable
  const double* g_power;   // [B]         nullable
  const double* g_strehl;  // [B]         nullable
  double* values;          // [B][n_obs + 2]  nullable
  double* cbuf;            // [B][MRW + MRS][2]  C / cscale
  double* cscale;          // [B]
  _Float16* cop16;         // fast handles: [n_etiles][step 2][re|im][hi|lo][64][8], table 16 s + 8 (lane >> 5) + el of env lane & 31
  float* csci;             // fast handles: [Bp][2]  C_s / cscale
};

constexpr int kGradMaxTables = 80, kGradMaxOut = 1024 + 16;

__global__ __launch_bounds__(256) void k_grad_coef(GradCoefArgs p) {
#pragma clang fp contract(off)
  __shared__ double U[2 * kGradMaxTables], zr[kGradMaxOut + 1], zi[kGradMaxOut + 1], C[2 * kGradMaxTables];
  __shared__ double sc_sh;
  const int env = blockIdx.x, tid = threadIdx.x, MR = p.MRW + p.MRS;
  const size_t slab = (size_t)p.rows * p.Bp;
  for (int i = tid; i < 2 * MR; i += blockDim.x) {
    const int m = i >> 1, im = i & 1;
    const int row = m < p.MRW ? (im ? p.TW + m : m) : 2 * p.TW + (im ? p.TS : 0) + (m - p.MRW);
    double v = 0;
    for (int c = 0; c < p.n_chunks; ++c) v += p.slabs[c * slab + (size_t)row * p.Bp + env];
    U[i] = m < p.MRW ? v * p.inv_tscale : v;
  }
  __syncthreads();
  for (int j = tid; j <= p.n_out; j += blockDim.x) {
    double r = 0, s = 0;
    if (j < p.n_out) {
      const double* cf = p.wfs_coef + (size_t)j * p.MRW * 2;
      for (int m = 0; m < p.MRW; ++m) {
        r += cf[2 * m] * U[2 * m] - cf[2 * m + 1] * U[2 * m + 1];
        s += cf[2 * m] * U[2 * m + 1] + cf[2 * m + 1] * U[2 * m];
      }
    } else {
      for (int m = 0; m < p.MRS; ++m) {
        const double u = U[2 * (p.MRW + m)], v = U[2 * (p.MRW + m) + 1];
        r += p.sci_coef[2 * m] * u - p.sci_coef[2 * m + 1] * v;
        s += p.sci_coef[2 * m] * v + p.sci_coef[2 * m + 1] * u;
      }
    }
    zr[j] = r;
    zi[j] = s;
  }
  __syncthreads();
  if (p.values) {
    double* val = p.values + (size_t)env * (p.n_obs + 2);
    for (int j = tid; j < p.n_obs; j += blockDim.x) val[j] = p.n_obs_tab ? zr[j] * zr[j] + zi[j] * zi[j] : __builtin_nan("");
    if (tid == 0) {
      double power = 0;
      for (int j = p.n_obs_tab; j < p.n_out; ++j) power += zr[j] * zr[j] + zi[j] * zi[j];
      val[p.n_obs] = power;
      val[p.n_obs + 1] = zr[p.n_out] * zr[p.n_out] + zi[p.n_out] * zi[p.n_out];
    }
  }
  // C_m = sum_j gbar_j conj(Z_j) coef[j][m]
  const double gp = p.g_power ? p.g_power[env] : 0.0, gs = p.g_strehl ? p.g_strehl[env] : 0.0;
  for (int m = tid; m < MR; m += blockDim.x) {
    double cr = 0, ci = 0;
    if (m < p.MRW) {
      for (int j = 0; j < p.n_out; ++j) {
        const double g = j < p.n_obs_tab ? (p.g_obs ? p.g_obs[(size_t)env * p.n_obs + j] : 0.0) : gp;
        if (g == 0.0) continue;
        const double a = p.wfs_coef[((size_t)j * p.MRW + m) * 2], b = p.wfs_coef[((size_t)j * p.MRW + m) * 2 + 1];
        cr += g * (zr[j] * a + zi[j] * b);
        ci += g * (zr[j] * b - zi[j] * a);
      }
    } else {
      const double a = p.sci_coef[2 * (m - p.MRW)], b = p.sci_coef[2 * (m - p.MRW) + 1];
      cr = gs * (zr[p.n_out] * a + zi[p.n_out] * b);
      ci = gs * (zr[p.n_out] * b - zi[p.n_out] * a);
    }
    C[2 * m] = cr;
    C[2 * m + 1] = ci;
  }
  __syncthreads();
  if (tid == 0) {
    double big = 0;
    for (int i = 0; i < 2 * MR; ++i) big = fmax(big, fabs(C[i]));
    // a power of two: the division below is exact
    sc_sh = (big > 0 && big < 1e300) ? exp2((double)ilogb(big)) : 1.0;
    p.cscale[env] = sc_sh;
  }
  __syncthreads();
  const double inv = 1.0 / sc_sh;
  for (int i = tid; i < 2 * MR; i += blockDim.x) {
    C[i] = C[i] * inv;
    p.cbuf[(size_t)env * MR * 2 + i] = C[i];
  }
  __syncthreads();
  if (p.cop16 == nullptr) return;
  // the env's column of the B operands: tables past MRW are zeros
  for (int i = tid; i < 64; i += blockDim.x) {
    const int m = i >> 1, ri = i & 1, s = m >> 4, kg = (m >> 3) & 1, el = m & 7;
    const float v = m < p.MRW ? (float)C[2 * m + ri] : 0.f;
    _Float16 hi, lo;
    split_f16(v, hi, lo);
    const size_t base = ((((size_t)(env >> 5) * 2 + s) * 2 + ri) * 2) * 64 + (kg * 32 + (env & 31));
    p.cop16[base * 8 + el] = hi;
    p.cop16[(base + 64) * 8 + el] = lo;
  }
  if (tid < 2) p.csci[2 * (size_t)env + tid] = (float)C[2 * p.MRW + tid];
}

// ---- float64 validation handles: one workgroup per env ----
// trig [B][n_ap][4]: cos / sin of phi, cos / sin of r phi (the backward kernel overwrites element 0 with q_p); slab rows as GradCoefArgs
// with TW = MRW, TS = MRS
__global__ __launch_bounds__(256) void k_grad_ref_forward(const double* __restrict__ modes64, const double* __restrict__ tabs64,
                                                          const double* __restrict__ psi64, const double* __restrict__ act_dm,
                                                          double* __restrict__ trig, double* __restrict__ slab, int n_ap, int A, int MRW, int MRS,
                                                          int Bp, double lambda_wfs, double ratio) {
  __shared__ double sm[8];
  __shared__ double sa[256];
  const int env = blockIdx.x, MR = MRW + MRS;
  pupil64_stage_act(act_dm, env, A, sa);
  double* tg = trig + (size_t)env * n_ap * 4;
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double surf = pupil64_surface(modes64, sa, p, A);
    const double rev = (psi64[(size_t)env * n_ap + p] + 4.0 * M_PI * surf) / (2.0 * M_PI * lambda_wfs), revs = rev * ratio;
    double sn, cs;
    sincospi(2.0 * (rev - rint(rev)), &sn, &cs);
    tg[4 * p] = cs;
    tg[4 * p + 1] = sn;
    sincospi(2.0 * (revs - rint(revs)), &sn, &cs);
    tg[4 * p + 2] = cs;
    tg[4 * p + 3] = sn;
  }
  __syncthreads();
  for (int m = 0; m < MR; ++m) {
    const int off = m < MRW ? 0 : 2;
    double u = 0, v = 0;
    for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
      const double g = tabs64[(size_t)p * MR + m];
      u = fma(tg[4 * p + off], g, u);
      v = fma(tg[4 * p + off + 1], g, v);
    }
    const double Us = block_reduce_sum(u, sm), Vs = block_reduce_sum(v, sm);
    if (threadIdx.x == 0) {
      const int ru = m < MRW ? m : 2 * MRW + (m - MRW), rv = m < MRW ? MRW + m : 2 * MRW + MRS + (m - MRW);
      slab[(size_t)ru * Bp + env] = Us;
      slab[(size_t)rv * Bp + env] = Vs;
    }
  }
}

__global__ __launch_bounds__(256) void k_grad_ref_backward(const double* __restrict__ modes64, const double* __restrict__ tabs64,
                                                           const double* __restrict__ cbuf, double* __restrict__ trig, double* __restrict__ slab,
                                                           int n_ap, int A, int MRW, int MRS, int Bp, double ratio) {
  __shared__ double sm[8];
  __shared__ double C[2 * kGradMaxTables];
  const int env = blockIdx.x, MR = MRW + MRS;
  for (int i = threadIdx.x; i < 2 * MR; i += blockDim.x) C[i] = cbuf[(size_t)env * MR * 2 + i];
  __syncthreads();
  double* tg = trig + (size_t)env * n_ap * 4;
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double* g = tabs64 + (size_t)p * MR;
    double hr = 0, hi = 0, kr = 0, ki = 0;
    for (int m = 0; m < MRW; ++m) { hr = fma(C[2 * m], g[m], hr); hi = fma(C[2 * m + 1], g[m], hi); }
    for (int m = MRW; m < MR; ++m) { kr = fma(C[2 * m], g[m], kr); ki = fma(C[2 * m + 1], g[m], ki); }
    tg[4 * p] = -2.0 * (tg[4 * p] * hi + tg[4 * p + 1] * hr) - 2.0 * ratio * (tg[4 * p + 2] * ki + tg[4 * p + 3] * kr);
  }
  __syncthreads();
  pupil64_mode_rows(modes64, tg, 4, slab, n_ap, A, Bp, env, sm);
}

// ---- slabs -> grad_act, and grad_action through action -> actuators (AO_env.py:119-120) ----
struct GradFinishArgs {
  const double* slabs;     // [n_chunks][rows][Bp]: row k = sum_p M_pk q_p at the operand scales
  const double* cscale;    // [B]
  const double* gram;      // [A][A]
  const float* action;     // [B][A]  (grad_action only)
  double* grad_act;        // [B][A]  nullable
  double* grad_action;     // [B][A]  nullable
  int n_chunks, rows, Bp, A;
  double factor;           // 4 pi / lambda_wfs over the operand scales
  double target;           // cfg.surface_rms_target
  // the observation's part on the separable route (k_gradient_obs.h; all null / 0 otherwise: the sums above are then the whole gradient)
  const double* slabs2;    // [n_chunks2][rows2][Bp]  nullable
  const double* cscale2;   // [B]  nullable (1)
  int n_chunks2, rows2;
  double factor2;
};

__global__ __launch_bounds__(256) void k_grad_finish(GradFinishArgs p) {
#pragma clang fp contract(off)
  __shared__ double gsh[256], vsh[256], Gv[256];
  __shared__ double dots[2];
  const int env = blockIdx.x, k = threadIdx.x;
  const size_t slab = (size_t)p.rows * p.Bp;
  double g = 0;
  if (k < p.A) {
    const double T = pupil_slab_sum(p.slabs, p.n_chunks, slab, k, p.Bp, env);
    g = (T * p.factor) * p.cscale[env];
    if (p.slabs2) {
      const size_t slab2 = (size_t)p.rows2 * p.Bp;
      const double T2 = pupil_slab_sum(p.slabs2, p.n_chunks2, slab2, k, p.Bp, env);
      g += (T2 * p.factor2) * (p.cscale2 ? p.cscale2[env] : 1.0);
    }
    if (p.grad_act) p.grad_act[(size_t)env * p.A + k] = g;
  }
  if (!p.grad_action) return;
  // v_k = a_k / (k + 10), n = sqrt(v' G v), act = c v / n:  dL/dv = (c / n) (g - (g . v) (G v) / n^2),  dL/da_k = (dL/dv)_k / (k + 10)
  if (k < p.A) {
    gsh[k] = g;
    vsh[k] = (double)p.action[(size_t)env * p.A + k] / (double)(k + 10);
  }
  __syncthreads();
  if (k < p.A) {
    double s = 0;
    for (int j = 0; j < p.A; ++j) s += p.gram[(size_t)k * p.A + j] * vsh[j];
    Gv[k] = s;
  }
  __syncthreads();
  if (k == 0) {
    double n2 = 0, gv = 0;
    for (int j = 0; j < p.A; ++j) {
      n2 += vsh[j] * Gv[j];
      gv += gsh[j] * vsh[j];
    }
    dots[0] = n2;
    dots[1] = gv;
  }
  __syncthreads();
  if (k < p.A) {
    const double n2 = dots[0], n = sqrt(n2);
    const double dv = (p.target / n) * (g - (dots[1] * Gv[k]) / n2);
    p.grad_action[(size_t)env * p.A + k] = dv / (double)(k + 10);
  }
}

}  // namespace aog
