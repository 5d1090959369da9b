// K12: residual wavefront statistics and the least-squares projection of the pupil phase onto the mirror's modes (aog_wavefront_truth).
//
// Per env, with u_p = psi_p + (M' a)_p the phase in revolutions of lambda_wfs exactly as the step kernels form it (fp32 screen tiles plus
// the split-f16 mode contraction), the three sums over the aperture
//     S = sum_p u_p,    Q = sum_p u_p^2,    T_k = sum_p M_pk u_p   (k < A)
// are everything the definition in include/aogym.h needs: w = lambda_wfs u, and k_wavefront_finish does the rest in float64.
//   k_wavefront_fit<A_PAD>   fast handles.  A wave owns one env tile (32 envs, actuator operands resident) and every fourth pixel tile of its
//       workgroup's chunk.  Per pixel tile: u on v_mfma_f32_32x32x16_f16 (three split products per 16 modes, as k_phase_mfma); u stays in the
//       accumulator registers, is split into f16 hi + lo and is the B operand of the second contraction as it lies — register 8 s + el of
//       half-wave h is pixel (el & 3) + 16 s + 8 (el >> 2) + 4 h of the tile, which is tab16's pixel order, so the modes are laid out as
//       k_fused_tab's tables are (wf_tab16: A = 32 mode rows, K = 16 pixels per step, three split products per step and 32-row block).
//       S and Q are formed on the vector unit in float64; the fp32 accumulators of T are added to float64 after every tile (32 pixels).
//       The four waves' sums are added in wave order through LDS and go to slab [chunk][A_PAD + 2][Bp]: no atomics.  Which tiles a chunk
//       holds depends on n_ptiles only, an env's sums on nothing but its own column of the operands: a batch split over two handles gives
//       the bits of the whole batch.  No transcendental instruction, no B x n_ap intermediate.
//       (The mode operands of a pixel tile are read again by every env tile; they come from the L2 / Infinity Cache like k_fused_tab's, whose
//       loop order this is.  The screens, the only stream from HBM, are read once.)
//   k_wavefront_ref          float64 validation handles, in the style of k_fused_ref: one workgroup per env, psi64 and modes64; its sums are
//       in metres already (one slab).
//   k_wavefront_finish       one workgroup per env: slabs added in chunk order, revolutions -> metres, b centred with the column sums,
//       c = P b, the four outputs.  No fused multiply-add where the definition has none.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kWfChunkTiles = 64;   // pixel tiles per workgroup (16 per wave); the chunk count is ceil(n_ptiles / 64) whatever the batch
__host__ __device__ inline int wavefront_chunks(int n_ptiles) { return (n_ptiles + kWfChunkTiles - 1) / kWfChunkTiles; }
// 32-row blocks of the modes-as-tables operand
__host__ __device__ constexpr int wavefront_blocks(int A_pad) { return (A_pad + 31) / 32; }

template <int A_PAD>
__global__ __launch_bounds__(256) void k_wavefront_fit(const f16x8* __restrict__ modes16, const f16x8* __restrict__ wf_tab16,
                                                       const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16,
                                                       double* __restrict__ slabs, int n_ptiles, int n_ap, int Bp) {
  constexpr int NSTEP = A_PAD / 16, NBLK = wavefront_blocks(A_PAD), ROWS = A_PAD + 2;
  __shared__ double red[ROWS * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int chunk = blockIdx.x, etile = blockIdx.y;
  // this env tile's actuator operands stay in registers
  f16x8 bh[NSTEP], bl[NSTEP];
  {
    const f16x8* asrc = act16 + ((size_t)etile * NSTEP * 2) * 64 + lane;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) { bh[s] = asrc[(2 * s) * 64]; bl[s] = asrc[(2 * s + 1) * 64]; }
  }
  double acc[NBLK][16];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] = 0.0;
  double acc_s = 0.0, acc_q = 0.0;
  const int t_end = min((chunk + 1) * kWfChunkTiles, n_ptiles);
  int t = chunk * kWfChunkTiles + wave;
  f32x4 pc[4], pn[4];
  auto load_psi = [&](int tile, f32x4 (&pp)[4]) {
    const size_t base = (((size_t)etile * n_ptiles + tile) * 4) * 64 + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) pp[g] = psi_tile[base + g * 64];
  };
  if (t < t_end) load_psi(t, pc);
  for (; t < t_end; t += 4) {   // (wave-uniform)
    if (t + 4 < t_end) load_psi(t + 4, pn);   // the next tile's screen values are requested ahead
    const f16x8* ms = modes16 + ((size_t)t * NSTEP * 2) * 64 + lane;
    f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      const f16x8 mh = ms[(2 * s) * 64], ml = ms[(2 * s + 1) * 64];
      d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bh[s], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bl[s], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml, bh[s], d, 0, 0, 0);
    }
    // u of this lane's 16 pixels (register 4 g + r: pixel 8 g + 4 h + r of the tile); pad pixels of the last tile are exact zeros
    const int left = n_ap - t * 32 - 4 * h;   // pixel 8 g + r of this half-wave is real iff 8 g + r < left
    f16x8 uh[2], ul[2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = fmaf(d[4 * g + r], kPhaseUnscale, pc[g][r]);
        const float u = (8 * g + r < left) ? v : 0.f;
        const double ud = (double)u;
        acc_s += ud;
        acc_q = fma(ud, ud, acc_q);
        const float sc = u * kActScale;   // (phases of a few revolutions: the operand scale of the actuators)
        const _Float16 hi = (_Float16)sc;
        uh[g >> 1][4 * (g & 1) + r] = hi;
        ul[g >> 1][4 * (g & 1) + r] = (_Float16)(sc - (float)hi);
      }
    // T += M' u: the phase is the B operand (K = the tile's 32 pixels in two steps), the modes the A operand in blocks of 32 rows
    const f16x8* ts = wf_tab16 + ((size_t)t * NBLK * 4) * 64 + lane;
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
      f32x16 D = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f16x8 th = ts[((b * 2 + s) * 2) * 64], tl = ts[((b * 2 + s) * 2 + 1) * 64];
        D = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, uh[s], D, 0, 0, 0);
        D = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ul[s], D, 0, 0, 0);
        D = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, uh[s], D, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[b][j] += (double)D[j];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) pc[g] = pn[g];
  }
  // the two half-waves hold different pixels of the same env
  acc_s += __shfl_down(acc_s, 32, 64);
  acc_q += __shfl_down(acc_q, 32, 64);
  // the four waves' sums in wave order (a wave without tiles adds zeros)
  constexpr double unscale = 1.0 / ((double)kModeScale * (double)kActScale);
  const int col = lane & 31;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int m = 32 * b + 8 * (j >> 2) + 4 * h + (j & 3);
          if (m < A_PAD) {
            const double v = acc[b][j] * unscale;
            red[m * 32 + col] = w == 0 ? v : red[m * 32 + col] + v;
          }
        }
      if (h == 0) {
        red[A_PAD * 32 + col] = w == 0 ? acc_s : red[A_PAD * 32 + col] + acc_s;
        red[(A_PAD + 1) * 32 + col] = w == 0 ? acc_q : red[(A_PAD + 1) * 32 + col] + acc_q;
      }
    }
    __syncthreads();
  }
  double* out = slabs + (size_t)chunk * ROWS * Bp + (size_t)etile * 32;
  for (int i = threadIdx.x; i < ROWS * 32; i += 256) out[(size_t)(i >> 5) * Bp + (i & 31)] = red[i];
}

// float64 validation form: one workgroup per env.  w (metres) goes through a work buffer of the call's own; the sums land in one slab
// [A_rows + 2][Bp] with the fast kernel's row order.
__global__ __launch_bounds__(256) void k_wavefront_ref(const double* __restrict__ modes64, const double* __restrict__ psi64,
                                                       const double* __restrict__ act_dm, double* __restrict__ w_buf,
                                                       double* __restrict__ slab, int n_ap, int A, int rows, int Bp) {
  __shared__ double sm[8];
  __shared__ double sa[256];
  const int env = blockIdx.x;
  for (int i = threadIdx.x; i < A; i += blockDim.x) sa[i] = act_dm[(size_t)env * A + i];
  __syncthreads();
  double* w = w_buf + (size_t)env * n_ap;
  double s = 0, q = 0;
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const double* mrow = modes64 + (size_t)p * A;
    double surf = 0;
    for (int k = 0; k < A; ++k) surf = fma(mrow[k], sa[k], surf);
    const double wp = psi64[(size_t)env * n_ap + p] / (2.0 * M_PI) + 2.0 * surf;
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
  for (int k = 0; k < A; ++k) {
    double v = 0;
    for (int p = threadIdx.x; p < n_ap; p += blockDim.x) v = fma(modes64[(size_t)p * A + k], w[p], v);
    const double T = block_reduce_sum(v, sm);
    if (threadIdx.x == 0) slab[(size_t)k * Bp + env] = T;
  }
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
