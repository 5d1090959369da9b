// K24: tomography.  (a) The projection of a front's residual wavefront onto a caller's shapes (aog_wavefront_project), a sibling of K12
// on the loop, contractions and reduction of k_pupil_tile.h; (b) the reconstructor and integrator of aog_tomo_update, a small float64 GEMM
// whose every product and sum is rounded on its own.
//
// (a) Per env, with u_p the phase in revolutions exactly as K12 forms it, the sums  S = sum_p u_p  and  T_k = sum_p S_kp u_p  (k < K) are
// all the definition in include/aogym_tomography.h needs; k_project_finish does the rest in float64.
//   k_wavefront_project<A_PAD, GBLK>  fast handles.  K reaches 512 rows = 16 blocks of 32, and acc[16][16] float64 does not fit in
//       registers: the rows are cut into groups of GBLK <= 4 blocks over gridDim.z (GBLK = 4 is K12's own accumulator count at A_pad = 128).
//       Every group forms u of its tiles again — three MFMAs per 16 modes against 6 GBLK for the contraction — and reads a table of its
//       own, packed per group by pack_tab16_rows, so pupil_modes_mfma runs as it stands.  The operand scale of the shapes is the upload's
//       (the largest |S| below 2^14); `unscale` takes it off together with kActScale.  Slab [group][chunk][32 GBLK + 1][Bp], last row S.
//   k_project_ref     float64 handles, in the style of k_wavefront_ref: one workgroup per env, w in metres through a work buffer.
//   k_project_finish  one workgroup per env: slabs added in chunk order, revolutions -> metres, centred with the row sums.
#pragma once
#include "k_pupil_tile.h"

namespace aog {

constexpr int kProjectMaxBlocks = 4;   // 32-row blocks per row group: acc[4][16] float64 = 128 VGPRs, as k_wavefront_fit<128>

template <int A_PAD, int GBLK>
__global__ __launch_bounds__(256) void k_wavefront_project(const f16x8* __restrict__ modes16, const f16x8* __restrict__ shape_tab16,
                                                           const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16,
                                                           double* __restrict__ slabs, int n_ptiles, int n_ap, int Bp, double unscale) {
  constexpr int NSTEP = A_PAD / 16, GROWS = 32 * GBLK, ROWS = GROWS + 1;
  __shared__ double red[ROWS * 32];
  // this group's table and slabs
  const f16x8* tab = shape_tab16 + (size_t)blockIdx.z * n_ptiles * GBLK * 4 * 64;
  double* gslabs = slabs + (size_t)blockIdx.z * gridDim.x * ROWS * Bp;
  double acc[GBLK][16];
#pragma unroll
  for (int b = 0; b < GBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] = 0.0;
  double acc_s = 0.0;
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
        acc_s += (double)u[4 * g + r];
      }
    f16x8 uh[2], ul[2];
    pupil_split16(u, kActScale, uh, ul);
    pupil_modes_mfma<GBLK>(tab, t, uh, ul, acc);
  });
  acc_s += __shfl_down(acc_s, 32, 64);   // the two half-waves hold different pixels of the same env
  pupil_reduce_store<ROWS>(red, gslabs, Bp, [&](auto put) __attribute__((always_inline)) {
    pupil_mode_rows<GROWS>(acc, [&](int m, double v) __attribute__((always_inline)) { put(m, v * unscale); });
    if (pupil_half() != 0) return;
    put(GROWS, acc_s);
  });
}

// float64 validation form: shapes64 [n_ap][K]; slab [K + 1][Bp], row K = sum_p w_p (metres)
__global__ __launch_bounds__(256) void k_project_ref(const double* __restrict__ modes64, const double* __restrict__ shapes64,
                                                     const double* __restrict__ psi64, const double* __restrict__ act_dm,
                                                     double* __restrict__ w_buf, double* __restrict__ slab, int n_ap, int A, int K, int Bp) {
  __shared__ double sm[8];
  __shared__ double sa[256];
  const int env = blockIdx.x;
  pupil64_stage_act(act_dm, env, A, sa);
  double* w = w_buf + (size_t)env * n_ap;
  double s = 0;
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double wp = psi64[(size_t)env * n_ap + p] / (2.0 * M_PI) + 2.0 * pupil64_surface(modes64, sa, p, A);
    w[p] = wp;
    s += wp;
  }
  const double S = block_reduce_sum(s, sm);
  if (threadIdx.x == 0) slab[(size_t)K * Bp + env] = S;
  __syncthreads();   // (w of the whole env is written)
  pupil64_mode_rows(shapes64, w, 1, slab, n_ap, K, Bp, env, sm);
}

struct ProjectFinishArgs {
  const double* slabs;     // [group][n_chunks][rows][Bp]: rows k < rows - 1 of group g = T of shape g (rows - 1) + k, row rows - 1 = S
  const double* rowsum;    // [K]
  double* out;             // [B][K]
  double* mean;            // [B] nullable
  int n_chunks, rows, Bp, K, n_ap;
  double scale;            // metres per unit of the sums (lambda_wfs for revolutions, 1 for the float64 kernel's)
};

__global__ __launch_bounds__(256) void k_project_finish(ProjectFinishArgs p) {
#pragma clang fp contract(off)
  const int env = blockIdx.x;
  const size_t slab = (size_t)p.rows * p.Bp;
  const double S = pupil_slab_sum(p.slabs, p.n_chunks, slab, p.rows - 1, p.Bp, env);   // (group 0's: every group holds the same bits)
  const double mean = (S * p.scale) / (double)p.n_ap;
  if (threadIdx.x == 0 && p.mean) p.mean[env] = mean;
  for (int k = threadIdx.x; k < p.K; k += blockDim.x) {
    const int g = k / (p.rows - 1), r = k - g * (p.rows - 1);
    const double T = pupil_slab_sum(p.slabs + (size_t)g * p.n_chunks * slab, p.n_chunks, slab, r, p.Bp, env);
    p.out[(size_t)env * p.K + k] = T * p.scale - p.rowsum[k] * mean;
  }
}

// ---- (b) the reconstructor and integrator ----
constexpr int kTomoEnvs = 32, kTomoOuts = 64, kTomoCols = 64, kTomoMaxInputs = 4;

struct TomoArgs {
  const double* R[kTomoMaxInputs];   // [K][J_g]
  const double* s[kTomoMaxInputs];   // [B][J_g]
  int J[kTomoMaxInputs];
  double* u;                         // [B][K]
  double* out;                       // [B][K] nullable
  const uint8_t* mask;               // [B] nullable
  int B, K, G;
  double gain, leak, stroke;
};

// Grid dim3(env tiles of 32, output tiles of 64), 256 threads: thread = output k0 + (t & 63) of the 8 envs b0 + 8 (t >> 6) + i.  Per
// input and per 64 columns the workgroup stages R [64][64 (+1: the lanes of a wave read a column)] and s [32][64] in LDS; a wave reads one
// R value per lane and 8 s values the whole wave shares per column.  acc runs over g, then j, in one thread: the order of a (b, k) sum
// is the same in every tiling.
__global__ __launch_bounds__(256) void k_tomo_update(TomoArgs a) {
  __shared__ double Rl[kTomoOuts][kTomoCols + 1];
  __shared__ double sl[kTomoEnvs][kTomoCols];
  const int b0 = blockIdx.x * kTomoEnvs, k0 = blockIdx.y * kTomoOuts;
  const int kk = threadIdx.x & 63, eg = threadIdx.x >> 6;
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0;
  for (int g = 0; g < a.G; ++g) {
    const int J = a.J[g];
    const double* __restrict__ R = a.R[g];
    const double* __restrict__ s = a.s[g];
    for (int j0 = 0; j0 < J; j0 += kTomoCols) {
      const int nj = min(kTomoCols, J - j0);
      __syncthreads();   // (the last chunk's reads are done)
      for (int i = threadIdx.x; i < kTomoOuts * kTomoCols; i += 256) {
        const int r = i >> 6, c = i & 63;
        Rl[r][c] = (k0 + r < a.K && c < nj) ? R[(size_t)(k0 + r) * J + j0 + c] : 0.0;
      }
      for (int i = threadIdx.x; i < kTomoEnvs * kTomoCols; i += 256) {
        const int r = i >> 6, c = i & 63;
        sl[r][c] = (b0 + r < a.B && c < nj) ? s[(size_t)(b0 + r) * J + j0 + c] : 0.0;
      }
      __syncthreads();
      for (int c = 0; c < nj; ++c) {   // (nj is uniform: a pad column never enters a sum)
        const double r = Rl[kk][c];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = add_rn(acc[i], mul_rn(r, sl[8 * eg + i][c]));
      }
    }
  }
  const int k = k0 + kk;
  if (k >= a.K) return;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = b0 + 8 * eg + i;
    if (b >= a.B) continue;
    const size_t at = (size_t)b * a.K + k;
    double v = a.u[at];
    if (!a.mask || a.mask[b]) {
      v = add_rn(mul_rn(a.leak, v), -mul_rn(a.gain, acc[i]));
      if (a.stroke > 0.0) {
        v = v < -a.stroke ? -a.stroke : v;
        v = v > a.stroke ? a.stroke : v;
      }
      a.u[at] = v;
    }
    if (a.out) a.out[at] = v;
  }
}

__global__ __launch_bounds__(256) void k_tomo_reset(double* u, const uint8_t* mask, int B, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  if (mask && !mask[i / K]) return;
  u[i] = 0.0;
}

}  // namespace aog
