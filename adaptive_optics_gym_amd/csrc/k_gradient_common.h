// K14: what the kernels of k_gradient.h and k_gradient_obs.h (two translation units) share — the pixel-chunk geometry of the backward
// contraction and the split of accumulator-order values into its B operand.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kGradChunkTiles = 64;     // pixel tiles per workgroup (16 per wave)
__host__ __device__ inline int grad_chunks(int n_ptiles) { return (n_ptiles + kGradChunkTiles - 1) / kGradChunkTiles; }
__host__ __device__ constexpr int grad_blocks(int A_pad) { return (A_pad + 31) / 32; }

// 16 accumulator-order values -> the B operand of a contraction over the tile's pixels (two K steps), hi + lo
__device__ __forceinline__ void grad_split16(const float (&v)[16], float scale, f16x8 (&hi)[2], f16x8 (&lo)[2]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float sc = v[j] * scale;
    const _Float16 h = (_Float16)sc;
    hi[j >> 3][j & 7] = h;
    lo[j >> 3][j & 7] = (_Float16)(sc - (float)h);
  }
}

}  // namespace aog
