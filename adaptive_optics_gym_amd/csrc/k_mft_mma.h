// The split-f16 complex matrix-core product of the Fraunhofer transforms, and the ONE definition of their two passes: mft_pass1 / mft_pass2
// are the bodies of K4's kernels (k_focal.h) and of the science camera's (k_science.h), which differ in a geometry policy and in pass 2's
// tail alone; K11 (k_obs.h, one wave per tile, no LDS) shares the register-level pieces.  Layouts: see k_focal.h.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kFocalTile = 4 * 64;   // f16x8 per operand tile
// hi = x rounded to nearest f16, lo = x - hi rounded to nearest: an unbiased 22-bit operand.  (The step kernel's cheaper split by mask
// truncates both halves; here the truncation error — a fixed non-linear function of cos / sin of the phase — showed up as ghost terms of
// 1e-7 of the peak amplitude, the whole error budget of a pixel 30 dB down; this path has the vector slots to round properly.)
__device__ __forceinline__ void split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 h = (_Float16)x[j];
    hi[j] = h;
    lo[j] = (_Float16)(x[j] - (float)h);
  }
}
__device__ __forceinline__ f16x8 neg8(f16x8 v) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(f16x8, __builtin_bit_cast(u32x4, v) ^ 0x80008000u);
}
// 8 phases of the grid (revolutions; kShOutside outside the aperture) -> the four parts of an E tile: e[] = re hi, re lo, im hi, im lo of
// e^{2 pi i w}, 0 outside
__device__ __forceinline__ void mft_e_tile(const float (&w)[8], f16x8 (&e)[4]) {
  float c[8], s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool in = w[j] < 1.5f;
    c[j] = in ? __builtin_amdgcn_cosf(w[j]) : 0.f;   // (the instructions take revolutions; sincospif changed nothing measurable)
    s[j] = in ? __builtin_amdgcn_sinf(w[j]) : 0.f;
  }
  split8(c, e[0], e[1]);
  split8(s, e[2], e[3]);
}
// the accumulators of one (x tile, v block) of pass 1 -> T', split and in pass 2's operand order: registers 8 s .. 8 s + 7 of a lane = the 8
// k-slots of k-step s of this x tile.  dst: the lane's slot of the pair's first tile
__device__ __forceinline__ void mft_store_t16(f16x8* __restrict__ dst, const f32x16& cr, const f32x16& ci) {
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
// one A tile (re hi, re lo, im hi, im lo) against a B tile (nbh, nbl = -Bi), all in registers: Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br
__device__ __forceinline__ void mft_cmul(f16x8 arh, f16x8 arl, f16x8 aih, f16x8 ail, const f16x8 (&b)[4], f16x8 nbh, f16x8 nbl, f32x16& cr, f32x16& ci) {
  // (the two accumulation chains alternate; small terms first)
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[1], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[3], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, b[0], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, nbl, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, b[1], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[0], cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, b[2], ci, 0, 0, 0);
  cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, nbh, cr, 0, 0, 0);
  ci = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, b[0], ci, 0, 0, 0);
}
// the same with the A tile in LDS ([part][lane])
__device__ __forceinline__ void focal_mma_tile(const f16x8* __restrict__ a_tile, int lane, const f16x8 (&b)[4], f16x8 nbh, f16x8 nbl, f32x16& cr, f32x16& ci) {
  mft_cmul(a_tile[0 * 64 + lane], a_tile[1 * 64 + lane], a_tile[2 * 64 + lane], a_tile[3 * 64 + lane], b, nbh, nbl, cr, ci);
}

// ---- the two passes (layouts and the arithmetic: k_focal.h) ----
// Geometry of the output side, nvb blocks of 32 columns.  MftFull (K4): nvb is a multiple of 4, so every wave's block exists and each
// test below folds away at compile time.  MftWindow (the science camera): any nvb — a wave whose block lies past the window still produces
// its A tile of every k-step (the four waves share that work) but issues no matrix instruction and stores nothing — and the `split` form
// for nvb <= 2, in which the four waves share the two blocks so that every wave multiplies.  Each (tile, block) product is the same
// instruction sequence in every form: the bits do not depend on it.
struct MftFull {
  static constexpr bool kFull = true;
  static constexpr int split = 0;
  int nvb;
};
struct MftWindow {
  static constexpr bool kFull = false;
  int nvb, split;
};

// The k-step loop both passes run.  Workgroup = 4 waves over ONE 128-row span: wave `wave` produces the span's A tile `wave` of the next
// k-step into LDS (produce(buf), from what load_a(ks) requested), every wave then multiplies the span's tiles [t0, t1) by its own B tile,
// tile ks of btab (L2-resident), if it is `live`.
template <class LoadA, class Produce>
__device__ __forceinline__ void mft_ksteps(const f16x8 (&a_lds)[2][4 * kFocalTile], const f16x8* __restrict__ btab, int nk, int lane, int t0, int t1, bool live,
                                           LoadA load_a, Produce produce, f32x16 (&cr)[4], f32x16 (&ci)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { cr[t][r] = 0.f; ci[t][r] = 0.f; }
  f16x8 b[4], bn[4];
  auto load_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = btab[(size_t)ks * kFocalTile + q * 64];
  };
  load_a(0);
  load_b(0, b);
  produce(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int nxt = min(ks + 1, nk - 1);
    // the loads of the coming k-step go out BEFORE this k-step's matrix instructions (left alone the compiler sinks them to their first
    // use, after the matrix instructions, and every k-step then waits a full memory round trip between two bursts of matrix work;
    // requesting two k-steps ahead: no gain)
    load_a(nxt);
    load_b(nxt, bn);
    __builtin_amdgcn_sched_barrier(0);
    if (live) {
      const f16x8 nbh = neg8(b[2]), nbl = neg8(b[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t >= t0 && t < t1) focal_mma_tile(a_lds[ks & 1] + t * kFocalTile, lane, b, nbh, nbl, cr[t], ci[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    produce((ks + 1) & 1);   // (unconditional: under `if (ks + 1 < nk)` the loads above are sunk into the branch, behind the matrix instructions; the last
                             // k-step re-produces its own tile into the buffer nobody reads any more)
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bn[q];
    __syncthreads();
  }
}

// pass 1:  T'^T[x][v] = sum_y E[y][x] m1'[v][y], E formed from the phase grid while it is loaded (8 loads, 16 transcendentals and the split
// per lane and k-step).  grid (Nxp / 128, ceil(nvb / 4), envs); phase [env][Nyp][Nxp]; m1s [nvb][Nyp / 16] tiles; T16 [env][Nxp / 32][nvb][2] tiles.
// split: wave takes block wave & 1 against x tiles 2 (wave >> 1), + 1 of the span.
template <class G>
__device__ __forceinline__ void mft_pass1(const float* __restrict__ phase, const f16x8* __restrict__ m1s, f16x8* __restrict__ T16, int Nxp, int Nyp, G g) {
  __shared__ f16x8 a_lds[2][4 * kFocalTile];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int env = blockIdx.z, x0 = blockIdx.x * 128, vb = g.split ? (wave & 1) : blockIdx.y * 4 + wave;
  const int t0 = g.split ? 2 * (wave >> 1) : 0, t1 = g.split ? t0 + 2 : 4;   // x tiles of the span this wave multiplies
  const bool live = G::kFull || vb < g.nvb;   // (wave-uniform)
  const int nk = Nyp / 16;
  const float* __restrict__ src = phase + ((size_t)env * Nyp + 8 * (lane >> 5)) * Nxp + x0 + 32 * wave + (lane & 31);
  float w[8];   // phases of the k-step being produced next
  auto load_w = [&](int ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = src[(size_t)(ks * 16 + j) * Nxp];
  };
  auto produce = [&](int buf) {   // this wave's x tile of the k-step whose phases are in w -> LDS
    f16x8 e[4];
    mft_e_tile(w, e);
    f16x8* dst = a_lds[buf] + wave * kFocalTile + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q * 64] = e[q];
  };
  f32x16 cr[4], ci[4];
  mft_ksteps(a_lds, m1s + (size_t)(G::kFull ? vb : min(vb, g.nvb - 1)) * nk * kFocalTile + lane, nk, lane, t0, t1, live, load_w, produce, cr, ci);
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t >= t0 && t < t1) {
      const int xt = (x0 >> 5) + t;
      mft_store_t16(T16 + ((((size_t)env * (Nxp / 32) + xt) * g.nvb + vb) * 2) * kFocalTile + lane, cr[t], ci[t]);
    }
}

// pass 2:  F[v][u] = sum_x T'[v][x] m2'[x][u]; tail(env, u, v, re, im) takes every element of the n x n output, still scaled by 2^(e1 + e2).
// grid (ceil(nvb / 4) [u], ceil(nvb / 4) [v], envs); m2s [nvb][Nxp / 32][2] tiles.  k-step ks = (x tile ks >> 1, s = ks & 1); a workgroup
// multiplies the nt = min(4, nvb - vb0) v blocks that exist, wave `wave` copying the T' tile of v block vb0 + wave.
// split: wave takes u block wave & 1 against v block wave >> 1 alone.
// (fp32 sums over the whole of x.  Folding them into float64 every one or two k-steps was built and measured: worst error 0.84 -> 0.45 of
// K4's test tolerance at N = 256, but 384 accumulator registers mean one wave per SIMD and the kernel went from 100 to 250 us.)
template <class G, class Tail>
__device__ __forceinline__ void mft_pass2(const f16x8* __restrict__ T16, const f16x8* __restrict__ m2s, int Nxp, int n, G g, Tail tail) {
  __shared__ f16x8 a_lds[2][4 * kFocalTile];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int env = blockIdx.z, ub = g.split ? (wave & 1) : blockIdx.x * 4 + wave, vb0 = blockIdx.y * 4;
  const int nt = G::kFull ? 4 : min(4, g.nvb - vb0), nk = (Nxp / 32) * 2;
  const int t0 = g.split ? (wave >> 1) : 0, t1 = g.split ? t0 + 1 : nt;   // v blocks of the span this wave multiplies
  const bool live = G::kFull || ub < g.nvb, feeds = G::kFull || wave < nt;   // (wave-uniform) this wave multiplies / copies a tile
  const f16x8* __restrict__ asrc = T16 + ((size_t)env * (Nxp / 32) * g.nvb + vb0 + (G::kFull ? wave : min(wave, nt - 1))) * 2 * kFocalTile + lane;
  f16x8 a[4];
  auto load_a = [&](int ks) {
    const f16x8* p = asrc + ((size_t)(ks >> 1) * g.nvb * 2 + (ks & 1)) * kFocalTile;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = p[q * 64];
  };
  auto produce = [&](int buf) {
    if (!feeds) return;
    f16x8* dst = a_lds[buf] + wave * kFocalTile + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q * 64] = a[q];
  };
  f32x16 cr[4], ci[4];
  mft_ksteps(a_lds, m2s + (size_t)(G::kFull ? ub : min(ub, g.nvb - 1)) * nk * kFocalTile + lane, nk, lane, t0, t1, live, load_a, produce, cr, ci);
  const int u = ub * 32 + (lane & 31);
  if (!live || u >= n) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t >= t0 && t < t1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = (vb0 + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (v < n) tail(env, u, v, cr[t][r], ci[t][r]);
      }
    }
}

}  // namespace aog
