// K23: the altitude mirror (include/aogym_conjugate.h).  k_altmirror_surface turns commands into surfaces on the meta-pupil, a
// [B, K] x [K, M M] float64 product whose every output element is the header's chain of rounded products and sums in mode order;
// k_altmirror_fit contracts a layer's logical screen with the fit matrix.
#pragma once
#include "k_common.h"
#include "k_layers.h"   // layer_phys: the one definition of a ring's logical -> physical pixel

namespace aog {

// One workgroup = kSurfEnvs envs x kSurfPixels pixels.  A lane holds pixels p and p + 256 of its 8 envs (16 float64 sums), so one basis
// value it loads — coalesced along p — serves 8 envs; the 8 commands of mode k are wave-uniform (scalar loads).  Workgroups that share a
// pixel chunk are neighbours in the grid (the env group varies fastest), so a chunk's K basis rows (8 K x 512 bytes) are fetched into
// L2 once per chunk and device, not once per env group.  Pad envs of a ragged last group compute env B - 1 again and store nothing; a
// group with no selected env returns at once.
constexpr int kSurfEnvs = 8;
constexpr int kSurfPixels = 512;   // 2 per lane
// cmd [B][K] -> surface [B][MM] (and, `command` non-null, the record [B][K]) of the envs `mask` (nullable) selects
__global__ __launch_bounds__(256) void k_altmirror_surface(const double* __restrict__ basis, const double* __restrict__ cmd, const uint8_t* __restrict__ mask,
                                                           double* __restrict__ command, double* __restrict__ surface, int B, int K, int MM, int n_groups) {
  const int chunk = blockIdx.x / n_groups, group = blockIdx.x - chunk * n_groups;
  const int env0 = group * kSurfEnvs;
  bool on[kSurfEnvs], any = false;
  const double* c[kSurfEnvs];
#pragma unroll
  for (int e = 0; e < kSurfEnvs; ++e) {
    const int env = min(env0 + e, B - 1);
    on[e] = env0 + e < B && (!mask || mask[env]);
    any = any || on[e];
    c[e] = cmd + (size_t)env * K;
  }
  if (!any) return;   // uniform
  const int p[2] = {chunk * kSurfPixels + (int)threadIdx.x, chunk * kSurfPixels + 256 + (int)threadIdx.x};
  const int pc[2] = {min(p[0], MM - 1), min(p[1], MM - 1)};
  double s[kSurfEnvs][2];
  {
    const double b0 = basis[pc[0]], b1 = basis[pc[1]];
#pragma unroll
    for (int e = 0; e < kSurfEnvs; ++e) {
      const double ce = c[e][0];
      s[e][0] = mul_rn(ce, b0);
      s[e][1] = mul_rn(ce, b1);
    }
  }
  for (int k = 1; k < K; ++k) {
    const double* row = basis + (size_t)k * MM;
    const double b0 = row[pc[0]], b1 = row[pc[1]];
#pragma unroll
    for (int e = 0; e < kSurfEnvs; ++e) {
      const double ce = c[e][k];
      s[e][0] = add_rn(s[e][0], mul_rn(ce, b0));
      s[e][1] = add_rn(s[e][1], mul_rn(ce, b1));
    }
  }
#pragma unroll
  for (int e = 0; e < kSurfEnvs; ++e) {
    if (!on[e]) continue;   // uniform
    double* out = surface + (size_t)(env0 + e) * MM;
    if (p[0] < MM) out[p[0]] = s[e][0];
    if (p[1] < MM) out[p[1]] = s[e][1];
    if (command && chunk == 0)
      for (int k = threadIdx.x; k < K; k += 256) command[(size_t)(env0 + e) * K + k] = c[e][k];
  }
}

// cmd_out[b][k] = sum_p fit[k][p] screen_b[p] over the logical screen.  One workgroup = one env x kFitModes modes: a thread reads its
// strided pixels of the screen once (through the env's ring origin) for 8 modes, then block_reduce_sum per mode — a fixed order, no
// atomics, the same bits in any batch (as k_layer_mean).
constexpr int kFitModes = 8;
__global__ __launch_bounds__(256) void k_altmirror_fit(const double* __restrict__ fit, const double* __restrict__ master, const int32_t* __restrict__ origin,
                                                       double* __restrict__ cmd_out, int K, int M) {
  __shared__ double sm[8];
  const int env = blockIdx.x, k0 = blockIdx.y * kFitModes;
  const int ox = origin[2 * env], oy = origin[2 * env + 1];
  const int MM = M * M;
  const double* screen = master + (size_t)env * MM;
  const double* row[kFitModes];
#pragma unroll
  for (int j = 0; j < kFitModes; ++j) row[j] = fit + (size_t)min(k0 + j, K - 1) * MM;
  double acc[kFitModes] = {};
  for (int p = threadIdx.x; p < MM; p += 256) {
    const int iy = p / M, ix = p - iy * M;
    const double v = screen[layer_phys(iy, ix, oy, ox, M)];
#pragma unroll
    for (int j = 0; j < kFitModes; ++j) acc[j] += row[j][p] * v;
  }
#pragma unroll
  for (int j = 0; j < kFitModes; ++j) {
    const double total = block_reduce_sum(acc[j], sm);
    if (threadIdx.x == 0 && k0 + j < K) cmd_out[(size_t)env * K + k0 + j] = total;
  }
}

}  // namespace aog
