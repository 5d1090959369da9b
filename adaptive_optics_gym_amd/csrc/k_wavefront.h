// K12: residual wavefront statistics and the least-squares projection of the pupil phase onto the mirror's modes (aog_wavefront_truth).
//
// Per env, with u_p = psi_p + (M' a)_p the phase in revolutions of lambda_wfs exactly as the step kernels form it (fp32 screen tiles plus
// the split-f16 mode contraction), the three sums over the aperture
//     S = sum_p u_p,    Q = sum_p u_p^2,    T_k = sum_p M_pk u_p   (k < A)
// are everything the definition in include/aogym.h needs: w = lambda_wfs u, and k_wavefront_finish does the rest in float64.
//   k_wavefront_fit<A_PAD>   fast handles, on the loop, contractions and reduction of k_pupil_tile.h.  Per pixel tile: u (pupil_phase_mfma) stays in
//       the accumulator registers, is split at the actuators' operand scale and is the B operand of the modes contraction as it lies
//       (wf_tab16).  S and Q are formed on the vector unit in float64.  Slab [chunk][A_PAD + 2][Bp]: rows k = T_k, A_PAD = S, A_PAD + 1 = Q.
//       No transcendental instruction, no B x n_ap intermediate.
//       (The mode operands of a pixel tile are read again by every env tile; they come from the L2 / Infinity Cache like k_fused_tab's, whose
//       loop order this is.  The screens, the only stream from HBM, are read once.)
//   k_wavefront_ref          float64 validation handles, in the style of k_fused_ref: one workgroup per env, psi64 and modes64; its sums are
//       in metres already (one slab).
//   k_wavefront_finish       one workgroup per env: slabs added in chunk order, revolutions -> metres, b centred with the column sums,
//       c = P b, the four outputs.  No fused multiply-add where the definition has none.
#pragma once
#include "k_pupil_tile.h"

namespace aog {

template <int A_PAD>
__global__ __launch_bounds__(256) void k_wavefront_fit(const f16x8* __restrict__ modes16, const f16x8* __restrict__ wf_tab16,
                                                       const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16,
                                                       double* __restrict__ slabs, int n_ptiles, int n_ap, int Bp) {
  constexpr int NSTEP = A_PAD / 16, NBLK = pupil_blocks(A_PAD), ROWS = A_PAD + 2;
  __shared__ double red[ROWS * 32];
  double acc[NBLK][16];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] = 0.0;
  double acc_s = 0.0, acc_q = 0.0;
  f16x8 bh[NSTEP], bl[NSTEP];
  pupil_tile_loop<NSTEP>(psi_tile, act16, n_ptiles, bh, bl, [&](int t, const f32x4 (&pc)[4]) {
    const f32x16 d = pupil_phase_mfma<NSTEP>(modes16, t, bh, bl);
    float u[16];
    const int left = pupil_left(n_ap, t);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = fmaf(d[4 * g + r], kPhaseUnscale, pc[g][r]);
        u[4 * g + r] = (8 * g + r < left) ? v : 0.f;   // pad pixels of the last tile are exact zeros
        const double ud = (double)u[4 * g + r];
        acc_s += ud;
        acc_q = fma(ud, ud, acc_q);
      }
    f16x8 uh[2], ul[2];
    pupil_split16(u, kActScale, uh, ul);   // (phases of a few revolutions: the operand scale of the actuators)
    pupil_modes_mfma<NBLK>(wf_tab16, t, uh, ul, acc);
  });
  // the two half-waves hold different pixels of the same env
  acc_s += __shfl_down(acc_s, 32, 64);
  acc_q += __shfl_down(acc_q, 32, 64);
  constexpr double unscale = 1.0 / ((double)kModeScale * (double)kActScale);
  pupil_reduce_store<ROWS>(red, slabs, Bp, [&](auto put) __attribute__((always_inline)) {
    pupil_mode_rows<A_PAD>(acc, [&](int m, double v) __attribute__((always_inline)) { put(m, v * unscale); });
    if (pupil_half() != 0) return;
    put(A_PAD, acc_s);
    put(A_PAD + 1, acc_q);
  });
}

// float64 validation form: one workgroup per env.  w (metres) goes through a work buffer of the call's own; the sums land in one slab
// [A_rows + 2][Bp] with the fast kernel's row order.
__global__ __launch_bounds__(256) void k_wavefront_ref(const double* __restrict__ modes64, const double* __restrict__ psi64,
                                                       const double* __restrict__ act_dm, double* __restrict__ w_buf,
                                                       double* __restrict__ slab, int n_ap, int A, int rows, int Bp) {
  __shared__ double sm[8];
  __shared__ double sa[256];
  const int env = blockIdx.x;
  pupil64_stage_act(act_dm, env, A, sa);
  double* w = w_buf + (size_t)env * n_ap;
  double s = 0, q = 0;
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double wp = psi64[(size_t)env * n_ap + p] / (2.0 * M_PI) + 2.0 * pupil64_surface(modes64, sa, p, A);
    w[p] = wp;
    s += wp;
    q = fma(wp, wp, q);
  }
  const double S = block_reduce_sum(s, sm), Q = block_reduce_sum(q, sm);
  if (threadIdx.x == 0) {
    slab[(size_t)(rows - 2) * Bp + env] = S;
    slab[(size_t)(rows - 1) * Bp + env] = Q;
  }
  __syncthreads();   // (w of the whole env is written)
  pupil64_mode_rows(modes64, w, 1, slab, n_ap, A, Bp, env, sm);
}

struct WavefrontFinishArgs {
  const double* slabs;     // [n_chunks][rows][Bp]: rows k < A = T_k, rows - 2 = S, rows - 1 = Q
  const double* fit;       // [A][A] P (symmetric)
  const double* colsum;    // [A]
  const double* act_dm;    // [B][A]
  double* rms;             // [B]     nullable
  double* fit_rms;         // [B]     nullable
  double* coef;            // [B][A]  nullable
  double* act_ideal;       // [B][A]  nullable
  int n_chunks, rows, Bp, A, n_ap;
  double scale;            // metres per unit of the sums (lambda_wfs for revolutions, 1 for the float64 kernel's)
};

__global__ __launch_bounds__(256) void k_wavefront_finish(WavefrontFinishArgs p) {
#pragma clang fp contract(off)
  __shared__ double bs[256], cs[256];
  const int env = blockIdx.x, k = threadIdx.x;
  const size_t slab = (size_t)p.rows * p.Bp;
  double S = 0, Q = 0, T = 0;
  for (int c = 0; c < p.n_chunks; ++c) {
    S += p.slabs[c * slab + (size_t)(p.rows - 2) * p.Bp + env];
    Q += p.slabs[c * slab + (size_t)(p.rows - 1) * p.Bp + env];
    if (k < p.A) T += p.slabs[c * slab + (size_t)k * p.Bp + env];
  }
  const double n = (double)p.n_ap;
  const double mean = (S * p.scale) / n;
  const double var = fmax(0.0, ((Q * p.scale) * p.scale) / n - mean * mean);
  if (k < p.A) bs[k] = T * p.scale - p.colsum[k] * mean;   // b = Mc' w
  __syncthreads();
  if (k < p.A) {
    double c = 0;
    for (int j = 0; j < p.A; ++j) c += p.fit[(size_t)j * p.A + k] * bs[j];   // (P is symmetric: row j read along k)
    cs[k] = c;
    if (p.coef) p.coef[(size_t)env * p.A + k] = c;
    if (p.act_ideal) p.act_ideal[(size_t)env * p.A + k] = p.act_dm[(size_t)env * p.A + k] - c * 0.5;
  }
  __syncthreads();
  if (k == 0) {
    if (p.rms) p.rms[env] = sqrt(var);
    if (p.fit_rms) {
      double dot = 0;
      for (int j = 0; j < p.A; ++j) dot += bs[j] * cs[j];
      p.fit_rms[env] = sqrt(fmax(0.0, var - dot / n));
    }
  }
}

}  // namespace aog
