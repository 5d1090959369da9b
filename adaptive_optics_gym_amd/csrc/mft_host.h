// Host side of the two-pass matrix Fourier transform family (K4, K11, K13, K14's observation part, K15 and its gradient): the split-f16
// operand tiles and their two K orders, the padded pupil geometry, the work buffers and the float64 validation chain (DESIGN.md §5,
// "Operand tiles of the MFT family").  Host-only: no kernel header includes it.  Implementations: focal.hip.
#pragma once
#include "host_common.h"

#include <complex>

namespace aog_host {

// One tile = [re hi, re lo, im hi, im lo][lane 64][8] f16 (kFocalTile f16x8 on the device).  A table holds a matrix m [i][k] (i: the row or
// column a lane carries, k: the contraction index) as [i >> 5][k >> 4] tiles, k_pad / 16 per 32-block, with k in one of two orders
// (AOG_TILE_NATURAL, AOG_TILE_ACCUMULATOR):
//   natural       lane (i & 31) + 32 ((k >> 3) & 1), slot k & 7
//   accumulator   lane (i & 31) + 32 ((k >> 2) & 1), slot (k & 3) + 4 ((k >> 3) & 1): k-step s of a 32 of k holds, in register order, the
//                 rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 8 s + slot, of a 32 x 32 matrix-core accumulator
constexpr size_t kTilePartF16 = 64 * 8, kTileF16 = 4 * kTilePartF16;
struct TilePos { int block, kstep, lane, slot; };
inline TilePos tile_pos_natural(int i, int k) { return {i >> 5, k >> 4, (i & 31) + 32 * ((k >> 3) & 1), k & 7}; }
inline TilePos tile_pos_accumulator(int i, int k) { return {i >> 5, k >> 4, (i & 31) + 32 * ((k >> 2) & 1), (k & 3) + 4 * ((k >> 3) & 1)}; }
// f16 of a [n_blocks][k_pad / 16] table, and where part 0 of element (i, k) lies in it (the other parts follow kTilePartF16 apart)
inline size_t operand_f16(int n_blocks, int k_pad) { return (size_t)n_blocks * (k_pad / 16) * kTileF16; }
inline size_t tile_offset(int order, int k_pad, int i, int k) {
  const TilePos p = order == AOG_TILE_NATURAL ? tile_pos_natural(i, k) : tile_pos_accumulator(i, k);
  return ((size_t)p.block * (k_pad / 16) + p.kstep) * kTileF16 + (size_t)p.lane * 8 + p.slot;
}
// The four parts of an element: a complex float64 is split here (hi through float, round to nearest like the kernels' split8; lo from the
// float64 remainder of the hi that came out), parts that are split already are copied.  (Host code is compiled with contraction on, so the
// two conversions may be merged into one rounding: a value within float rounding of a half tie can get the other neighbour as its hi than
// a two-step conversion gives.  Either split carries the value.)
struct TileParts { _Float16 part[4]; };
inline TileParts tile_parts(const TileParts& p) { return p; }
inline TileParts tile_parts(std::complex<double> c) {
  TileParts p;
  const double v[2] = {c.real(), c.imag()};
  for (int q = 0; q < 2; ++q) {
    p.part[2 * q] = (_Float16)(float)v[q];
    p.part[2 * q + 1] = (_Float16)(float)(v[q] - (double)(float)p.part[2 * q]);
  }
  return p;
}
// dst [n_blocks][k_pad / 16] tiles in `order` <- element(i, k) (std::complex<double> or TileParts) for i < rows, k < K; the pads are zero
template <typename F>
void pack_tiles(_Float16* dst, int order, int n_blocks, int k_pad, int rows, int K, F&& element) {
  std::fill(dst, dst + operand_f16(n_blocks, k_pad), (_Float16)0.f);
  for (int i = 0; i < std::min(rows, 32 * n_blocks); ++i)
    for (int k = 0; k < std::min(K, k_pad); ++k) {
      const TileParts p = tile_parts(element(i, k));
      _Float16* d = dst + tile_offset(order, k_pad, i, k);
      for (int q = 0; q < 4; ++q) d[q * kTilePartF16] = p.part[q];
    }
}
// dst <- the transposed matrix of the packed table src, in another order and shape: element (i, k) of dst is element (k, i) of src, parts
// copied (nothing is rounded again); zero where src has no such element
void reorder_tiles(_Float16* dst, int dst_order, int dst_blocks, int dst_k_pad, const _Float16* src, int src_order, int src_blocks, int src_k_pad);
// the power of two that brings the largest of n components into [1/2, 1) (1 for an all-zero or non-finite table)
double scale_of(const double* v, size_t n);

inline const aog::f16x8* f16x8p(const _Float16* p) { return reinterpret_cast<const aog::f16x8*>(p); }
inline aog::f16x8* f16x8p(_Float16* p) { return reinterpret_cast<aog::f16x8*>(p); }

// The padded pupil grid of a transform and the 32-blocks of its focal window: y to whole 16-row k-steps; x to the 128-column spans of pass 1
// (mft_geom_wide: K4, K13, K15) or to whole 32-column tiles, one wave each, with one window block (mft_geom_narrow: K11, K14)
inline int blocks32(int n) { return (n + 31) / 32; }
struct MftGeom {
  int Nxp, Nyp, nvb;
  size_t grid_env() const { return (size_t)Nyp * Nxp; }       // floats of one env's phase grid
  size_t m1_f16() const { return operand_f16(nvb, Nyp); }     // f16 of one transform's m1s (lane v, K = y natural),
  size_t m2_f16() const { return operand_f16(nvb, Nxp); }     //   of its m2s (lane u, K = x accumulator)
  size_t t16_env() const { return operand_f16(nvb, Nxp); }    //   and of one env's T16
};
inline MftGeom mft_geom_wide(int N, int window) { return {round_up(N, 128), round_up(N, 16), blocks32(window)}; }
inline MftGeom mft_geom_narrow(int N) { return {round_up(N, 32), round_up(N, 16), 1}; }
// m1s and m2s of a Fraunhofer matrix Fourier transform m1 [nf][N] . E . m2 [N][nf], each matrix scaled by scale_of; returns the unscale
// factor 2^-(e1 + e2)
float mft_operand_tables(const double* m1, const double* m2, int N, int nf, const MftGeom& g, std::vector<_Float16>& m1s, std::vector<_Float16>& m2s);

// The work buffers of a transform.  The chunk is the handle's whole env tiles, capped at cap_envs (the caller's memory rule) rounded down to
// whole tiles, at least one, and at the value of the environment variable chunk_env (nullable; tests: several chunks at small sizes); the
// grid starts out as "outside the aperture" everywhere (only aperture pixels are ever written).  Blocking.
int mft_work_alloc(aog_env* e, MftWork* w, size_t grid_env, size_t t16_env, size_t cap_envs, const char* chunk_env);
// a feature's own actuator operands (load_actuators' act16 and act_ll, either nullable), zeroed; buffers that are there already stay
int alloc_act_operands(aog_env* e, _Float16** act16, _Float16** act_ll);

// The steps of the float64 validation forms for one env.  launch_focal_field: E = exp(2 pi i ratio u_p) on the aperture pixels of the
// [N][N] complex grid E (the rest is left as it is); launch_cgemm64: out [R][Cn] (and / or its complex64 copy out32) = a [R][K] b [K][Cn],
// complex row-major.  mask (nullable): nothing happens for an env it leaves out.  act_src: nullable [B][A] actuators instead of the mirror's.
void launch_focal_field(aog_env* e, hipStream_t s, double* E, int env, double ratio = 1.0, const uint8_t* mask = nullptr, const double* act_src = nullptr);
void launch_cgemm64(hipStream_t s, const double* a, const double* b, double* out, float* out32, int R, int K, int Cn, const uint8_t* mask = nullptr, int env = 0);
// One transform's float64 tables and scratch, m1 [w][N], m2 [N][w], E [N][N], T [w][N] complex, and its chain E -> T = m1 E -> F = T m2
// [w][w] for one env (F and / or its complex64 copy F32).  field = false: E holds the env's field already (the pyramid's further points)
struct Mft64 { const double *m1, *m2; double *E, *T; int w; };
void launch_mft64(aog_env* e, hipStream_t s, const Mft64& t, double* F, float* F32, int env, bool field = true, double ratio = 1.0,
                  const uint8_t* mask = nullptr, const double* act_src = nullptr);

}  // namespace aog_host
