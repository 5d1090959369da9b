// Launch geometry and dynamic-LDS layout of the fused pupil pass: the one definition that the constructor (aog_create), the launchers
// (fused_inst.hip) and the kernel (k_fused_tab, k_fused.h) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>

namespace aog {

constexpr size_t kLdsBytes = 160 * 1024;   // LDS per CU on gfx950

// k_fused_tab's table sums sit in 32x32 accumulators: registers a < tab_live_regs(MRW) hold real tables
__host__ __device__ constexpr int tab_live_regs(int MRW) { return MRW <= 8 ? 4 : (MRW <= 16 ? 8 : (MRW <= 24 ? 12 : 16)); }
// few tables: the float64 sums of those registers stay in registers; beyond, every wave keeps them in a plane of LDS
__host__ __device__ constexpr bool tab_f64_in_regs(int MRW) { return MRW <= 8; }

// Dynamic LDS of one k_fused_tab workgroup, in bytes from its start.  Areas in this order:
//   sci [max_tiles][h 2][4] float4                   science table of the chunk's pixel tiles in accumulator order (every variant)
//   op  [waves][A_PAD / 16][hi|lo][64 lanes] f16x8   each wave's actuator operands (A_PAD > 64 or ring-direct: short of registers)
//   xp  [waves][32 envs][kXpRow] float               each wave's transpose tile of the ring-direct loads (ring-direct only)
//   acc [waves][2 live][64 lanes] double             each wave's float64 table sums (many-table variants only), 16-byte aligned
struct FusedLds {
  static constexpr int kSciVecs = 2 * 4;        // float4 per pixel tile
  static constexpr int kSciTile = kSciVecs * 16;
  static constexpr int kOpStep = 2 * 64 * 16;   // per wave and 16 modes
  static constexpr int kXpRow = 36;             // floats per env row: 32 pixels and 4 of padding
  static constexpr int kXpWave = 32 * kXpRow * 4;
  static constexpr int kAccReg = 2 * 64 * 8;    // per wave and live accumulator register (cos and sin)
  int sci_bytes, op_off, op_wave, op_bytes, xp_off, xp_bytes, acc_off, acc_wave, acc_bytes, total;
  __host__ __device__ constexpr FusedLds(int max_tiles, int waves, int A_PAD, int MRW, bool ring_direct)
      : sci_bytes(max_tiles * kSciTile),
        op_off(sci_bytes),
        op_wave(A_PAD / 16 * kOpStep),
        op_bytes((A_PAD > 64 || ring_direct) ? waves * op_wave : 0),
        xp_off(op_off + op_bytes),
        xp_bytes(ring_direct ? waves * kXpWave : 0),
        acc_off((xp_off + xp_bytes + 15) / 16 * 16),
        acc_wave(tab_live_regs(MRW) * kAccReg),
        acc_bytes(tab_f64_in_regs(MRW) ? 0 : waves * acc_wave),
        total(acc_off + acc_bytes) {}
  // Longest chunk (pixel tiles) whose science rows fit beside the other areas; <= 0: those alone are too large.  aog_create caps the tiles
  // per chunk with it before it knows whether the handle will run ring-direct (aog_upload_tables decides that), so every dynamic handle
  // counts as one, and the transpose tiles are counted whenever the operands are.  The cap decides the chunk count and with it the order
  // of the float64 sums: it is part of the numerical contract and stays as it is, the 64 bytes of slack included (every other term is a
  // multiple of kSciTile, so the slack makes the cap one tile less than an exact fit).
  static constexpr int tile_budget(int waves, int A_PAD, int MRW, bool atm_dynamic) {
    const int fixed = FusedLds(0, waves, A_PAD, MRW, A_PAD > 64 || atm_dynamic).total + 64;
    const int fit = ((int)kLdsBytes - fixed) / kSciTile;
    return fit < 4096 ? fit : 4096;
  }
  // Longest chunk that fits beside the areas of the layout that is actually launched: a static handle never holds transpose tiles, a
  // dynamic one counts as ring-direct (the larger of its two forms).  No slack.  Never below tile_budget.
  static constexpr int tile_fit(int waves, int A_PAD, int MRW, bool atm_dynamic) {
    const int fit = ((int)kLdsBytes - FusedLds(0, waves, A_PAD, MRW, atm_dynamic).total) / kSciTile;
    return fit < 4096 ? fit : 4096;
  }
  // The cap fused_geometry applies: tile_budget wherever it is positive (the shapes that always launched keep their chunk counts); where it
  // is not, because it counts transpose tiles that a static A_PAD = 128 handle does not have, tile_fit.  <= 0: no chunk fits this form.
  static constexpr int tile_cap(int waves, int A_PAD, int MRW, bool atm_dynamic) {
    const int budget = tile_budget(waves, A_PAD, MRW, atm_dynamic);
    return budget > 0 ? budget : tile_fit(waves, A_PAD, MRW, atm_dynamic);
  }
  // whether fused_geometry may choose `waves` waves per workgroup for this variant
  static constexpr bool form_fits(int waves, int A_PAD, int MRW, bool atm_dynamic) { return tile_cap(waves, A_PAD, MRW, atm_dynamic) > 0; }
};

// every variant the library instantiates: the areas follow each other without overlap on 16-byte boundaries; every form fused_geometry
// can choose for a variant (8 waves only where form_fits, 4 waves everywhere) has a positive cap, and a chunk as long as the cap allows
// fits the CU's LDS whether or not the handle turns out ring-direct
constexpr bool fused_lds_sound() {
  for (int waves = 4; waves <= 8; waves += 4)
    for (int A_PAD = 16; A_PAD <= 128; A_PAD *= 2)
      for (int MRW : {7, 12, 20, 28})
        for (int dyn = 0; dyn < 3; ++dyn) {   // static, dynamic through psi_tile, ring-direct
          const int tiles = FusedLds::tile_cap(waves, A_PAD, MRW, dyn > 0);
          const bool chosen = waves == 4 || FusedLds::form_fits(waves, A_PAD, MRW, dyn > 0);
          if (chosen && tiles <= 0) return false;
          if (tiles < FusedLds::tile_budget(waves, A_PAD, MRW, dyn > 0) || tiles > FusedLds::tile_fit(waves, A_PAD, MRW, dyn > 0)) return false;
          const FusedLds l(tiles > 0 ? tiles : 1, waves, A_PAD, MRW, dyn == 2);
          if (l.op_off < l.sci_bytes || l.xp_off < l.op_off + l.op_bytes || l.acc_off < l.xp_off + l.xp_bytes || l.total < l.acc_off + l.acc_bytes) return false;
          if (l.op_off % 16 || l.xp_off % 16 || l.acc_off % 16) return false;
          if (chosen && (size_t)l.total > kLdsBytes) return false;
        }
  return true;
}
static_assert(fused_lds_sound(), "k_fused_tab's LDS areas overlap, are misaligned, exceed the cap they were sized by, or a form that can be chosen has no room for a chunk");

// Launch geometry of the fused kernels.  The chunk counts and the tiles per chunk fix the order of the float64 sums, so this is part of the
// numerical contract, not a tuning detail.
struct FusedGeom {
  int valu_qpc = 0, valu_chunks = 0;   // k_fused_valu: pixel quads per chunk, chunks
  // k_fused_tab (see MfmaGeom in k_fused.h)
  int we = 1;         // env tiles per workgroup
  int waves = 4;      // waves per workgroup (8 with asymmetric pairs)
  int heavy = 0;      // asymmetric wave pairs: share (x / 1024) of a chunk's tiles that the prioritised sub-chunk takes; 0 = off
  int wg_y = 0;       // workgroups that share a pixel chunk
  int pair = 0;       // 1: the two workgroups of a CU walk the same pixel chunk (fused_wg_map)
  int chunks_x = 0;   // pixel chunks
  int tpc = 0;        // max tiles of any chunk: ceil(n_ptiles / chunks_x)
  int n_chunks = 0;   // partial slabs the epilogue sums
};
// pixel_chunks: the caller's choice (cfg.pixel_chunks), 0 = automatic.  four_wave: keep 4-wave workgroups (AOG_FUSED_4WAVE).
// A variant whose 8-wave fixed areas leave no room for a chunk (FusedLds::form_fits) keeps 4-wave workgroups at every batch size.  The
// result's tpc can still exceed what the CU holds if no form fits at all: fused_geometry_fits says so, and aog_create refuses the shape.
constexpr FusedGeom fused_geometry(int Bp, int n_ap_pad, int A_pad, int MRW, bool mfma, bool atm_dynamic, int pixel_chunks, bool four_wave) {
  FusedGeom g;
  const int n_quads = n_ap_pad / 4, n_ptiles = n_ap_pad / 32, n_etiles = Bp / 32, n_groups = Bp / 64;
  // aim at ~3 (VALU) / ~2 (MFMA) waves per SIMD over 256 CUs
  const int P = pixel_chunks > 0 ? pixel_chunks : std::max(1, (256 * 4 * 3 + n_groups - 1) / n_groups);
  g.valu_qpc = ((n_quads + P - 1) / P + 7) / 8 * 8;
  g.valu_chunks = (n_quads + g.valu_qpc - 1) / g.valu_qpc;
  g.we = n_etiles >= 4 ? 4 : (n_etiles >= 2 ? 2 : 1);
  // Asymmetric wave pairs (see k_fused_tab): with at least 4 env tiles the kernel runs 8-wave workgroups, one per CU, whose two pixel
  // sub-chunks split a chunk about 2 : 1 with the priority on the larger share.  (Eight waves of the many-table variants need
  // 8 x 2 LIVE x 512 B of LDS — 128 KB at o = 5 — beside the chunk's science rows: one workgroup per CU, which is what this form runs.)
  const bool asym = mfma && n_etiles >= 4 && !four_wave && FusedLds::form_fits(8, A_pad, MRW, atm_dynamic);
  g.waves = asym ? 8 : 4;
  g.heavy = asym ? 672 : 0;
  g.wg_y = (n_etiles + g.we - 1) / g.we;
  g.pair = (g.waves == 4 && g.wg_y % 2 == 0 && 64 % g.wg_y == 0 && g.wg_y >= 2) ? 1 : 0;
  // P pixel chunks (proportional split of the tiles), 8 waves per CU when the batch allows.  Every variant keeps float64 sums, so a chunk
  // may be as long as its science rows fit in the LDS.
  int Pm = pixel_chunks > 0 ? pixel_chunks : std::max(1, (asym ? 256 : 256 * 2) / g.wg_y);
  const int max_tpc = FusedLds::tile_cap(g.waves, A_pad, MRW, atm_dynamic);
  if (max_tpc > 0) Pm = std::max(Pm, (n_ptiles + max_tpc - 1) / max_tpc);
  Pm = std::min(Pm, n_ptiles);
  g.chunks_x = Pm;
  g.tpc = (n_ptiles + Pm - 1) / Pm;
  g.n_chunks = mfma ? g.chunks_x * (g.waves / g.we) : g.valu_chunks;
  return g;
}
// whether the geometry's longest chunk fits the CU's LDS in every layout the handle may launch it with
constexpr bool fused_geometry_fits(const FusedGeom& g, int A_pad, int MRW, bool atm_dynamic) {
  return g.chunks_x >= 1 && g.tpc >= 1 && (size_t)FusedLds(g.tpc, g.waves, A_pad, MRW, atm_dynamic).total <= kLdsBytes;
}

// The shapes of BASELINE.md's configs 2 and 3 (n_ap = 51468 at N = 256, A = 64), pinned: a change of any of these numbers changes the order of
// the float64 sums and with it the last bits of every output.
constexpr bool geom_is(const FusedGeom& g, int we, int waves, int heavy, int wg_y, int pair, int chunks_x, int tpc, int n_chunks, int valu_qpc, int valu_chunks) {
  return g.we == we && g.waves == waves && g.heavy == heavy && g.wg_y == wg_y && g.pair == pair && g.chunks_x == chunks_x && g.tpc == tpc &&
         g.n_chunks == n_chunks && g.valu_qpc == valu_qpc && g.valu_chunks == valu_chunks;
}
static_assert(geom_is(fused_geometry(1024, 51488, 64, 7, true, false, 0, false), 4, 8, 672, 8, 0, 32, 51, 64, 72, 179), "config 2: B = 1024, o = 2");
static_assert(FusedLds(51, 8, 64, 7, false).total == 6528, "config 2");
static_assert(geom_is(fused_geometry(4096, 51488, 64, 28, true, false, 0, false), 4, 8, 672, 32, 0, 8, 202, 16, 272, 48), "config 3: B = 4096, o = 5");
static_assert(FusedLds(202, 8, 64, 28, false).acc_off == 25856 && FusedLds(202, 8, 64, 28, false).total == 156928, "config 3");
// A shape that runs 4-wave workgroups because its 8-wave fixed areas (184 320 bytes ring-direct) leave no room for a chunk: config 4 (dynamic
// atmosphere, B = 1024) with the 5 x 5 observation.  And a 128-mode shape that keeps 8 waves: its budget counts transpose tiles a static
// handle does not have (-32), its real layout fits, and it launched before the form was chosen by fit.
static_assert(!FusedLds::form_fits(8, 64, 28, true) && FusedLds::form_fits(4, 64, 28, true), "dynamic, A_pad = 64, 28 tables");
static_assert(geom_is(fused_geometry(1024, 51488, 64, 28, true, true, 0, false), 4, 4, 0, 8, 1, 64, 26, 64, 72, 179), "config 4 at o = 5: 4-wave form");
static_assert(FusedLds(26, 4, 64, 28, true).total == 120064, "config 4 at o = 5");
static_assert(FusedLds::tile_budget(8, 128, 7, false) == -32 && FusedLds::tile_cap(8, 128, 7, false) == 256, "static, A_pad = 128, 7 tables");
static_assert(geom_is(fused_geometry(1024, 51488, 128, 7, true, false, 0, false), 4, 8, 672, 8, 0, 32, 51, 64, 72, 179), "B = 1024, A_pad = 128, o = 2");
static_assert(FusedLds(51, 8, 128, 7, false).total == 137600, "B = 1024, A_pad = 128, o = 2");

}  // namespace aog
