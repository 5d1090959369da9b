// Layered atmosphere: the float64 master screens of up to 8 dynamic handles summed into the screen layouts of a quasi-static front handle.
// Three kernels, one per pass: k_layer_mean (the aperture mean of the sum), then k_layer_sum_tiles (fast MFMA fronts: psi_tile) or
// k_layer_sum_f64 (float64 validation fronts: psi64).  Each is a template over two things besides the layer count L:
//   Layers  how the sum of the layers at one pixel is read: LayerSources (every layer in the pupil plane, through its ring origin:
//           aog_install_layer_sum, aog_install_layer_sum_disturbed) or SightLayers (layers larger than the front, read bilinearly at a
//           sub-pixel shift per layer and env: aog_install_layer_sum_sightline).  LayerReader<L, Layers> is the reader of one env.
//           SightLayers derives from LayerSources, so a pass reads `origin` and `master` of either by the same text.
//   Terms   what is added inside the sum: NoTerms (nothing, and no code for it: aog_install_layer_sum) or ModalTerms (K >= 0 pupil shapes
//           with per-env coefficients, K at run time: the other two entry points).
//           A third reader, ConeLayers (k_cone.h: sources at finite range, aog_install_layer_sum_cone), is defined beside this file.
// layers.hip instantiates <LayerSources, NoTerms>, <LayerSources, ModalTerms>, <SightLayers, ModalTerms> and <ConeLayers, ModalTerms> for
// L = 1 .. 8.
#pragma once
#include "k_common.h"

namespace aog {

constexpr int kMaxLayers = 8;

// the layers of one installation, by value in the kernel arguments (every index into these arrays is a compile-time constant)
struct LayerSources {
  const double* master[kMaxLayers];    // [B][N * N] toroidal float64 screens
  const int32_t* origin[kMaxLayers];   // [B][2] (ox, oy): logical pixel (iy, ix) lives at ((iy + oy) mod N, (ix + ox) mod N)
};

// physical offset of logical pixel (iy, ix) in a ring with origin (ox, oy); each axis wraps on its own
__device__ __forceinline__ int layer_phys(int iy, int ix, int oy, int ox, int N) {
  int py = iy + oy, px = ix + ox;
  if (py >= N) py -= N;
  if (px >= N) px -= N;
  return py * N + px;
}

// s = master_0 + master_1 + ... in layer order at one pixel of one env (the one definition of that order in the pupil plane: the host
// restatement of the tests adds the layers like this)
template <int L>
__device__ __forceinline__ double layer_sum_at(const LayerSources& src, size_t env_base, int iy, int ix, const int (&oy)[L], const int (&ox)[L], int N) {
  double v[L];
#pragma unroll
  for (int l = 0; l < L; ++l) v[l] = src.master[l][env_base + layer_phys(iy, ix, oy[l], ox[l], N)];
  double s = v[0];
#pragma unroll
  for (int l = 1; l < L; ++l) s += v[l];
  return s;
}

// ---- along a sightline (include/aogym_sightline.h) ----
// Layer l has N_l >= N pixels (margin c_l = (N_l - N) / 2) and is read at the logical position (iy + c_l + sy, ix + c_l + sx), bilinearly;
// (sx, sy) belongs to (layer, env).  Per env and layer — wave-uniform, scalar loads — a LayerTap holds the integer part of the shift folded
// with the margin and the ring origin into one offset per axis, reduced modulo N_l, and the four weights; a pixel then costs four loads
// (two neighbouring pairs: the second of each pair hits the line of the first), four products and three sums.  (ox, oy)[L]: the env's
// ring origins.
struct LayerSight {
  const double* shift[kMaxLayers];   // [B][2] (sx, sy) of this layer, pixels
  int n[kMaxLayers];                 // N_l
  int c[kMaxLayers];                 // c_l
};
struct SightLayers : LayerSources {
  LayerSight sight;
};
struct LayerTap {
  int by0, by1, bx0, bx1;   // ring origins of the rows y0, y0 + 1 and the columns x0, x0 + 1 of front pixel (0, 0): each in [0, N_l)
  double gy, fy, gx, fx;    // 1 - fy, fy, 1 - fx, fx
};
// (v mod n) in [0, n) for any int v
__device__ __forceinline__ int ring_mod(int v, int n) {
  const int r = v % n;
  return r < 0 ? r + n : r;
}
template <int L>
__device__ __forceinline__ void load_taps(const LayerSight& sight, int env, const int (&oy)[L], const int (&ox)[L], LayerTap (&tap)[L]) {
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int n = sight.n[l];
    const double sx = sight.shift[l][2 * env], sy = sight.shift[l][2 * env + 1];
    const double x0 = floor(sx), y0 = floor(sy);
    tap[l].fx = sx - x0;
    tap[l].fy = sy - y0;
    tap[l].gx = 1.0 - tap[l].fx;
    tap[l].gy = 1.0 - tap[l].fy;
    tap[l].bx0 = ring_mod(ox[l] + sight.c[l] + (int)x0, n);
    tap[l].by0 = ring_mod(oy[l] + sight.c[l] + (int)y0, n);
    tap[l].bx1 = tap[l].bx0 + 1 == n ? 0 : tap[l].bx0 + 1;
    tap[l].by1 = tap[l].by0 + 1 == n ? 0 : tap[l].by0 + 1;
  }
}
// s = v_0 + v_1 + ... in layer order at front pixel (iy, ix) < N <= N_l of one env; every sample goes through layer_phys with a folded
// origin < N_l, so one conditional subtraction per axis suffices and every address lies inside the env's screen
template <int L>
__device__ __forceinline__ double sight_sum_at(const LayerSources& src, const LayerSight& sight, int env, int iy, int ix, const LayerTap (&tap)[L]) {
  double v[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int n = sight.n[l];
    const double* m = src.master[l] + (size_t)env * n * n;
    const double v00 = m[layer_phys(iy, ix, tap[l].by0, tap[l].bx0, n)], v01 = m[layer_phys(iy, ix, tap[l].by0, tap[l].bx1, n)];
    const double v10 = m[layer_phys(iy, ix, tap[l].by1, tap[l].bx0, n)], v11 = m[layer_phys(iy, ix, tap[l].by1, tap[l].bx1, n)];
    const double top = add_rn(mul_rn(tap[l].gx, v00), mul_rn(tap[l].fx, v01));
    const double bottom = add_rn(mul_rn(tap[l].gx, v10), mul_rn(tap[l].fx, v11));
    v[l] = add_rn(mul_rn(tap[l].gy, top), mul_rn(tap[l].fy, bottom));
  }
  double s = v[0];
#pragma unroll
  for (int l = 1; l < L; ++l) s = add_rn(s, v[l]);
  return s;
}

// ---- the reader of one env: built from the env's ring origins (ox, oy)[L], which every pass loads in its own text (wave-uniform where the
// env is: scalar loads); at(iy, ix) is the layer-ordered sum at front pixel (iy, ix), kInFlight the number of pixels a thread of pass 1
// requests together.  The origins are not loaded in here: loaded by an inlined function, the origin pointers are fetched out of the
// kernel arguments once at the kernel's entry and held, and k_layer_sum_tiles<4, LayerSources, NoTerms> then needs 137 VGPRs instead of 128
// (three waves per SIMD instead of four); see profiles/layer_install_refactor.md ----
template <int L, class Layers>
struct LayerReader;
template <int L>
struct LayerReader<L, LayerSources> {
  static constexpr int kInFlight = 8;   // x L loads
  const LayerSources& src;
  const int env, N;
  const int (&oy)[L], (&ox)[L];   // the pass's arrays
  __device__ __forceinline__ LayerReader(const LayerSources& layers, int env, int N, const int (&oy)[L], const int (&ox)[L]) : src(layers), env(env), N(N), oy(oy), ox(ox) {}
  __device__ __forceinline__ double at(int iy, int ix) const { return layer_sum_at<L>(src, (size_t)env * N * N, iy, ix, oy, ox, N); }
};
template <int L>
struct LayerReader<L, SightLayers> {
  static constexpr int kInFlight = 4;   // x 4 L loads
  const SightLayers& layers;
  const int env;
  LayerTap tap[L];
  __device__ __forceinline__ LayerReader(const SightLayers& layers, int env, int, const int (&oy)[L], const int (&ox)[L]) : layers(layers), env(env) {
    load_taps<L>(layers.sight, env, oy, ox, tap);
  }
  __device__ __forceinline__ double at(int iy, int ix) const { return sight_sum_at<L>(layers, layers.sight, env, iy, ix, tap); }
};

// ---- a modal disturbance added inside the sum (include/aogym_disturbance.h) ----
// At env b and packed aperture pixel p: s = the reader's sum, then s = s + coeff[b][k] basis[k][p] for k = 0 .. K - 1, each product rounded,
// then each sum (mul_rn / add_rn of k_common.h, never one fma: the host restatement is bit-exact).  The coefficients of an env are uniform
// over the wave that works on it (scalar loads); a basis row is read coalesced along p, once for all the envs or pixels a lane holds, and
// the K rows stay in L2 (8 K n_ap bytes, shared by every env).
constexpr int kMaxTerms = 8;
struct ModalTerms {
  const double* __restrict__ basis;   // [K][n_ap]
  const double* __restrict__ coeff;   // [B][K]
  int K, n_ap;
};
struct NoTerms {};
// s[j] += the K terms of env[j] at pixel p[j] (< n_ap), j < J
template <int J>
__device__ __forceinline__ void add_terms(const ModalTerms& terms, double (&s)[J], const int (&env)[J], const int (&p)[J]) {
  for (int k = 0; k < terms.K; ++k) {
    double b[J];
#pragma unroll
    for (int j = 0; j < J; ++j) b[j] = terms.basis[(size_t)k * terms.n_ap + p[j]];
#pragma unroll
    for (int j = 0; j < J; ++j) s[j] = add_rn(s[j], mul_rn(terms.coeff[(size_t)env[j] * terms.K + k], b[j]));
  }
}
template <int J>
__device__ __forceinline__ void add_terms(const NoTerms&, double (&)[J], const int (&)[J], const int (&)[J]) {}

// The leading kernel argument: the layers, then the terms.  NoTerms as an empty base takes no room, where as an argument of its own it
// would move every later argument by 8 bytes.
template <class Layers, class Terms>
struct LayerSum : Layers, Terms {};

// Pass 1: the aperture mean of this step's sum, one workgroup per env: per-thread strided sums, then block_reduce_sum (a fixed order, no
// atomics: the mean of an env is the same bits in whatever batch the env sits, and the order of a thread's additions is the same for
// either kInFlight).
template <int L, class Layers, class Terms>
__global__ __launch_bounds__(256) void k_layer_mean(LayerSum<Layers, Terms> sum, const int32_t* __restrict__ ap_index, double* __restrict__ mean, int N,
                                                     int n_ap) {
  constexpr int U = LayerReader<L, Layers>::kInFlight;
  __shared__ double sm[8];
  const int env = blockIdx.x;
  int oy[L], ox[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    ox[l] = sum.origin[l][2 * env];
    oy[l] = sum.origin[l][2 * env + 1];
  }
  const LayerReader<L, Layers> reader(sum, env, N, oy, ox);
  double acc = 0;
  for (int p0 = threadIdx.x; p0 < n_ap; p0 += U * (int)blockDim.x) {
    double s[U];
    int envs[U], pc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * (int)blockDim.x;
      envs[u] = env;
      pc[u] = p < n_ap ? p : n_ap - 1;
      const int flat = ap_index[pc[u]], iy = flat / N, ix = flat - iy * N;
      s[u] = reader.at(iy, ix);
    }
    add_terms(sum, s, envs, pc);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (p0 + u * (int)blockDim.x < n_ap) acc += s[u];
  }
  const double total = block_reduce_sum(acc, sm);
  if (threadIdx.x == 0) mean[env] = total / (double)n_ap;
}

// Pass 2, fast MFMA handles: k_repack_master's layout (k_extrude.h).  One workgroup = one 32-env tile x kLayerIters pairs of 32-pixel
// tiles; a wave gathers 64 consecutive packed pixels of its 8 envs from every layer (coalesced along x), the block transposes through a
// padded LDS tile and every wave writes whole 1-KiB rows of psi_tile.  Unlike the repack it subtracts the exact mean of THIS sum (pass 1)
// and accumulates nothing.  The staging row is 68 floats: the transposed float4 reads of lanes e = 0 .. 15 start 4 e banks apart (one
// 16-B slot each, 16 distinct slots of the 64-bank row), the row-wise 4-byte writes are consecutive.
// Pad pixels (p >= n_ap) and pad envs (>= B, whole pad env tiles included) are written as exact zeros.
constexpr int kLayerIters = 4;
template <int L, class Layers, class Terms>
__global__ __launch_bounds__(256) void k_layer_sum_tiles(LayerSum<Layers, Terms> sum, const int32_t* __restrict__ ap_index, const double* __restrict__ mean,
                                                          float* __restrict__ psi_tile, int B, int N, int n_ap, int n_ptiles, double inv_two_pi_lambda) {
  constexpr int LD = 68;
  __shared__ float stage[32 * LD];
  const int et = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int it = 0; it < kLayerIters; ++it) {
    const int pt0 = (blockIdx.x * kLayerIters + it) * 2;
    if (pt0 >= n_ptiles) break;   // uniform
    const int p = pt0 * 32 + lane;
    const bool valid_p = p < n_ap;
    const int pc1 = valid_p ? p : n_ap - 1;
    const int flat = ap_index[pc1];   // logical pupil coordinates of this lane's packed pixel (same for every env and layer)
    const int iy = flat / N, ix = flat - iy * N;
    double s[8];
    int envs[8], pc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {   // (the env, and with it the reader's state and the coefficients, is wave-uniform: scalar loads)
      const int env = min(et * 32 + wave * 8 + q, B - 1);
      int oy[L], ox[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    ox[l] = sum.origin[l][2 * env];
    oy[l] = sum.origin[l][2 * env + 1];
  }
  const LayerReader<L, Layers> reader(sum, env, N, oy, ox);
      envs[q] = env;
      pc[q] = pc1;
      s[q] = reader.at(iy, ix);
    }
    add_terms(sum, s, envs, pc);
    if (it) __syncthreads();   // the previous iteration's rows have left the staging tile
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = wave * 8 + q;
      const bool ok = valid_p && et * 32 + e < B;
      stage[e * LD + lane] = ok ? (float)((s[q] - mean[min(et * 32 + e, B - 1)]) * inv_two_pi_lambda) : 0.f;
    }
    __syncthreads();
    // rows of psi_tile: [et][pt][g][lane = 32 h + e][4]; this pass owns pt0, pt0 + 1 (8 rows); wave w writes rows 2w, 2w+1
    for (int rr = 0; rr < 2; ++rr) {
      const int row = wave * 2 + rr, tl = row >> 2, g = row & 3;
      const int pt = pt0 + tl;
      if (pt >= n_ptiles) continue;
      const int h = lane >> 5, e = lane & 31;
      const float* from = stage + e * LD + tl * 32 + 8 * g + 4 * h;
      reinterpret_cast<float4*>(psi_tile)[(((size_t)et * n_ptiles + pt) * 4 + g) * 64 + lane] = make_float4(from[0], from[1], from[2], from[3]);
    }
  }
}

// Pass 2, float64 validation handles: psi64 [B][n_ap] = s - mean in hcipy's units, one workgroup per env
template <int L, class Layers, class Terms>
__global__ __launch_bounds__(256) void k_layer_sum_f64(LayerSum<Layers, Terms> sum, const int32_t* __restrict__ ap_index, const double* __restrict__ mean,
                                                        double* __restrict__ psi64, int N, int n_ap) {
  const int env = blockIdx.x;
  int oy[L], ox[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    ox[l] = sum.origin[l][2 * env];
    oy[l] = sum.origin[l][2 * env + 1];
  }
  const LayerReader<L, Layers> reader(sum, env, N, oy, ox);
  const double mu = mean[env];
  for (int p = threadIdx.x; p < n_ap; p += blockDim.x) {
    const int flat = ap_index[p], iy = flat / N, ix = flat - iy * N;
    double s[1] = {reader.at(iy, ix)};
    const int envs[1] = {env}, pc[1] = {p};
    add_terms(sum, s, envs, pc);
    psi64[(size_t)env * n_ap + p] = s[0] - mu;
  }
}

}  // namespace aog
