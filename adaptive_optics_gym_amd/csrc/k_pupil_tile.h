// What the off-step pupil kernels share — K12 (k_wavefront.h) and K14 (k_gradient.h, k_gradient_obs.h; three translation units): the loop of
// a wave over the pixel tiles of its workgroup's chunk, the two split-f16 contractions on v_mfma_f32_32x32x16_f16 with the register order
// they leave, the reduction of the four waves into a slab, and the float64 forms of the validation handles.  One definition each.
//
// Geometry.  Grid dim3(pixel chunks, env tiles), 256 threads.  A workgroup owns one env tile (32 envs) and one chunk of kPupilChunkTiles pixel
// tiles (32 packed aperture pixels each); its wave w takes tiles chunk * 64 + w, + 4, ...  Which tiles a chunk holds depends on n_ptiles
// only and an env's sums on nothing but its own column of the operands: a batch split over two handles gives the bits of the whole batch.
// The last chunk may hold fewer than four tiles; a wave without tiles runs no iteration, loads nothing, and adds the zeros its accumulators
// start with.
//
// Register order.  Every matrix product here has the envs of the tile along the lanes (column = lane & 31) and 32 rows — pixels of the tile, or
// rows of a 32-row block — in the 16 accumulator registers of the two half-waves h = lane >> 5: register j = 4 g + r is row 8 g + 4 h + r
// (pupil_acc_row).  The K = 16 elements of a B operand are, for k-step s and half-wave h, element el <-> K index 16 s + 8 h + el of lane's
// column.  Split as they lie (pupil_split16: registers 8 s .. 8 s + 7 are k-step s), 16 accumulator values are therefore the B operand of a
// contraction over the tile's pixels in the order: element el of k-step s, half-wave h <-> pixel (el & 3) + 16 s + 8 (el >> 2) + 4 h, which
// is tab16's pixel order (k_fused_tab's tables).  The host packs the A operands of such a contraction in that order (pack_tab16_rows):
// no LDS, no transposition between the two contractions.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kPupilChunkTiles = 64;   // pixel tiles per workgroup (16 per wave); the chunk count is ceil(n_ptiles / 64) whatever the batch
constexpr int kPupilWaves = 4;
__host__ __device__ inline int pupil_chunks(int n_ptiles) { return (n_ptiles + kPupilChunkTiles - 1) / kPupilChunkTiles; }
// 32-row blocks of the modes-as-tables operand
__host__ __device__ constexpr int pupil_blocks(int A_pad) { return (A_pad + 31) / 32; }
// row (pixel of the tile, or row of a 32-row block) that accumulator register j of half-wave h holds
__host__ __device__ constexpr int pupil_acc_row(int j, int h) { return 8 * (j >> 2) + 4 * h + (j & 3); }

// ---- the tile loop ----
// this wave's tiles of the workgroup's chunk: t, t + kPupilWaves, ... < t_end (wave-uniform)
struct PupilTileRange { int t, t_end; };
__device__ __forceinline__ PupilTileRange pupil_tile_range(int n_ptiles) {
  const int chunk = blockIdx.x, wave = threadIdx.x >> 6;
  return {chunk * kPupilChunkTiles + wave, min((chunk + 1) * kPupilChunkTiles, n_ptiles)};
}
// body(t) per tile: for kernels that read neither screens nor actuators (k_grad_obs_backward)
template <typename Body>
__device__ __forceinline__ void pupil_for_tiles(int n_ptiles, Body&& body) {
  const PupilTileRange r = pupil_tile_range(n_ptiles);
  for (int t = r.t; t < r.t_end; t += kPupilWaves) body(t);
}
// body(t, pc) per tile, pc = the screen values (revolutions) of the lane's 16 pixels, pc[g][r] = register 4 g + r.  The env tile's actuator
// operands are loaded into bh / bl first and stay in registers; the next tile's screen values are requested one tile ahead.
template <int NSTEP, typename Body>
__device__ __forceinline__ void pupil_tile_loop(const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16, int n_ptiles, f16x8 (&bh)[NSTEP],
                                                f16x8 (&bl)[NSTEP], Body&& body) {
  const int lane = threadIdx.x & 63, etile = blockIdx.y;
  {
    const f16x8* asrc = act16 + ((size_t)etile * NSTEP * 2) * 64 + lane;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) { bh[s] = asrc[(2 * s) * 64]; bl[s] = asrc[(2 * s + 1) * 64]; }
  }
  const PupilTileRange r = pupil_tile_range(n_ptiles);
  f32x4 pc[4], pn[4];
  auto load_psi = [&](int tile, f32x4 (&pp)[4]) {
    const size_t base = (((size_t)etile * n_ptiles + tile) * 4) * 64 + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) pp[g] = psi_tile[base + g * 64];
  };
  if (r.t < r.t_end) load_psi(r.t, pc);
  for (int t = r.t; t < r.t_end; t += kPupilWaves) {   // (wave-uniform)
    if (t + kPupilWaves < r.t_end) load_psi(t + kPupilWaves, pn);
    body(t, pc);
#pragma unroll
    for (int g = 0; g < 4; ++g) pc[g] = pn[g];
  }
}

// ---- the contractions ----
// (M' a) of the lane's 16 pixels of tile t at the operand scales: three split products per 16 modes (hi hi, hi lo, lo hi).  The caller takes the
// scales off in one fused multiply-add with the screen value, u = fmaf(d[4 g + r], kPhaseUnscale, pc[g][r]): revolutions exactly as the
// step kernels form them.
template <int NSTEP>
__device__ __forceinline__ f32x16 pupil_phase_mfma(const f16x8* __restrict__ modes16, int t, const f16x8 (&bh)[NSTEP], const f16x8 (&bl)[NSTEP]) {
  const f16x8* ms = modes16 + ((size_t)t * NSTEP * 2) * 64 + (threadIdx.x & 63);
  f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    const f16x8 mh = ms[(2 * s) * 64], ml = ms[(2 * s + 1) * 64];
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bh[s], d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh, bl[s], d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml, bh[s], d, 0, 0, 0);
  }
  return d;
}
// the half-wave h of this lane
__device__ __forceinline__ int pupil_half() { return (threadIdx.x & 63) >> 5; }
// pixel 8 g + r of this half-wave's registers (register 4 g + r) is a real aperture pixel iff 8 g + r < pupil_left(...): the last tile is ragged
__device__ __forceinline__ int pupil_left(int n_ap, int t) { return n_ap - t * 32 - 4 * pupil_half(); }

// 16 accumulator-order values -> the B operand of a contraction over the tile's pixels (two K steps), hi + lo
__device__ __forceinline__ void pupil_split16(const float (&v)[16], float scale, f16x8 (&hi)[2], f16x8 (&lo)[2]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float sc = v[j] * scale;
    const _Float16 h = (_Float16)sc;
    hi[j >> 3][j & 7] = h;
    lo[j >> 3][j & 7] = (_Float16)(sc - (float)h);
  }
}

// acc += M' q for pixel tile t: q is the B operand (K = the tile's 32 pixels in two steps), the modes the A operand in NBLK blocks of 32 rows
// (mtab16: pack_tab16_rows' layout), three split products per step; the fp32 sums of the tile's 32 pixels are added to float64 at once.
template <int NBLK>
__device__ __forceinline__ void pupil_modes_mfma(const f16x8* __restrict__ mtab16, int t, const f16x8 (&qh)[2], const f16x8 (&ql)[2],
                                                 double (&acc)[NBLK][16]) {
  const f16x8* mt = mtab16 + ((size_t)t * NBLK * 4) * 64 + (threadIdx.x & 63);
#pragma unroll
  for (int b = 0; b < NBLK; ++b) {
    f32x16 D = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f16x8 th = mt[((b * 2 + s) * 2) * 64], tl = mt[((b * 2 + s) * 2 + 1) * 64];
      D = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, qh[s], D, 0, 0, 0);
      D = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ql[s], D, 0, 0, 0);
      D = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, qh[s], D, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[b][j] += (double)D[j];
  }
}
// put(m, acc[b][j]) for the mode rows m < A_PAD this lane's accumulators hold
template <int A_PAD, int NBLK, typename Put>
__device__ __forceinline__ void pupil_mode_rows(const double (&acc)[NBLK][16], Put&& put) {
  const int h = pupil_half();
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int m = 32 * b + pupil_acc_row(j, h);
      if (m < A_PAD) put(m, acc[b][j]);
    }
}

// ---- the four waves' sums -> slab [chunk][ROWS][Bp] ----
// rows(put) names the (row, value) pairs of this lane's env with put(row, value); every row < ROWS is named by exactly one lane per env in
// every wave.  The waves add in wave order through red [ROWS * 32] (wave 0 writes, the others add): no atomics, and the same bits
// whatever the order in which the waves arrive.
template <int ROWS, typename Rows>
__device__ __forceinline__ void pupil_reduce_store(double* red, double* __restrict__ slabs, int Bp, Rows&& rows) {
  const int wave = threadIdx.x >> 6, col = threadIdx.x & 31;
  for (int w = 0; w < kPupilWaves; ++w) {
    if (wave == w) rows([&](int row, double v) __attribute__((always_inline)) { red[row * 32 + col] = w == 0 ? v : red[row * 32 + col] + v; });
    __syncthreads();
  }
  double* out = slabs + (size_t)blockIdx.x * ROWS * Bp + (size_t)blockIdx.y * 32;
  for (int i = threadIdx.x; i < ROWS * 32; i += 256) out[(size_t)(i >> 5) * Bp + (i & 31)] = red[i];
}

// row k of env's column summed over the slabs [n_chunks][rows][Bp] in chunk order (slab = rows * Bp): what every finish kernel starts from
__device__ __forceinline__ double pupil_slab_sum(const double* __restrict__ slabs, int n_chunks, size_t slab, int k, int Bp, int env) {
  double T = 0;
  for (int c = 0; c < n_chunks; ++c) T += slabs[c * slab + (size_t)k * Bp + env];
  return T;
}

// ---- float64 validation forms: one workgroup per env, modes64 [n_ap][A] ----
// the env's actuators (metres of surface) into sa [A] (a barrier follows), then the mirror surface at pixel p
__device__ __forceinline__ void pupil64_stage_act(const double* __restrict__ act_dm, int env, int A, double* sa) {
  for (int i = threadIdx.x; i < A; i += blockDim.x) sa[i] = act_dm[(size_t)env * A + i];
  __syncthreads();
}
__device__ __forceinline__ double pupil64_surface(const double* __restrict__ modes64, const double* sa, int p, int A) {
  const double* mrow = modes64 + (size_t)p * A;
  double surf = 0;
  for (int k = 0; k < A; ++k) surf = fma(mrow[k], sa[k], surf);
  return surf;
}
// row k of the slab = sum_p M_pk q[p * stride] for every k < A (q of the whole env written and a barrier passed); sm [8]
__device__ __forceinline__ void pupil64_mode_rows(const double* __restrict__ modes64, const double* q, int stride, double* __restrict__ slab, int n_ap,
                                                  int A, int Bp, int env, double* sm) {
  for (int k = 0; k < A; ++k) {
    double v = 0;
    for (int p = threadIdx.x; p < n_ap; p += blockDim.x) v = fma(modes64[(size_t)p * A + k], q[(size_t)p * stride], v);
    const double T = block_reduce_sum(v, sm);
    if (threadIdx.x == 0) slab[(size_t)k * Bp + env] = T;
  }
}

}  // namespace aog
