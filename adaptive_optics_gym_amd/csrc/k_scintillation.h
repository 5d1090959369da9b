// K26: scintillation (include/aogym_scintillation.h).  Around hipFFT's two transforms per layer: k_scint_pack (the mirror extension of
// a layer's logical screen), k_scint_multiply (the host-built (cos, sin) table) and k_scint_unpack (S - phi and chi on the meta-pupil).
// k_scint_install sums the chi surfaces at a front's shifts with the installation kernels' own bilinear read (LayerReader<L, SightLayers>
// of k_layers.h) into a float32 map in psi_tile's order; k_scint_receive is a reader of pupil_tile_loop (k_pupil_tile.h) that forms the
// residual phase as k_wavefront_fit does and adds the amplitude-weighted overlaps in float64; k_scint_finish turns the slabs into outputs.
#pragma once
#include "k_layers.h"
#include "k_pupil_tile.h"

namespace aog {

constexpr int kScintFiber = 4;               // receive-mode slots of the wmodes table (AOG_SCINT_MAX_FIBER)
constexpr int kScintRows = 2 * kScintFiber + 6;   // slab rows: Re c_k, Im c_k (k < 4), Re / Im of the on-axis sum, sum a, sum a^2, sum chi, sum chi^2

// index of the mirror extension: i < M itself, else 2 M - 1 - i (i < 2 M)
__device__ __forceinline__ int scint_mirror(int i, int M) { return i < M ? i : 2 * M - 1 - i; }

// work[e][y][x] = (phi_{env0 + e} at the mirrored logical pixel, 0): grid (ceil(E E / 256), chunk envs), E = 2 M
__global__ __launch_bounds__(256) void k_scint_pack(const double* __restrict__ master, const int32_t* __restrict__ origin, double2* __restrict__ work,
                                                    int env0, int M) {
  const int E = 2 * M, e = blockIdx.y, env = env0 + e;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * E) return;
  const int y = i / E, x = i - y * E;
  const int ox = origin[2 * env], oy = origin[2 * env + 1];
  const double v = master[(size_t)env * M * M + layer_phys(scint_mirror(y, M), scint_mirror(x, M), oy, ox, M)];
  work[(size_t)e * E * E + i] = make_double2(v, 0.0);
}

// work[e][f] *= (cos_f + i sin_f): the table's values, one complex product (each part a rounded product pair and sum)
__global__ __launch_bounds__(256) void k_scint_multiply(const double2* __restrict__ filter, double2* __restrict__ work, int EE) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= EE) return;
  const double2 f = filter[i];
  double2* w = work + (size_t)blockIdx.y * EE + i;
  const double2 v = *w;
  *w = make_double2(v.x * f.x - v.y * f.y, v.x * f.y + v.y * f.x);
}

// corr[env][p] = Re work / E^2 - phi, chi[env][p] = Im work / E^2 over the first M x M pixels of the extension, logical order
__global__ __launch_bounds__(256) void k_scint_unpack(const double2* __restrict__ work, const double* __restrict__ master, const int32_t* __restrict__ origin,
                                                      double* __restrict__ corr, double* __restrict__ chi, int env0, int M, double inv_n) {
  const int E = 2 * M, e = blockIdx.y, env = env0 + e;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M * M) return;
  const int y = p / M, x = p - y * M;
  const int ox = origin[2 * env], oy = origin[2 * env + 1];
  const double2 w = work[(size_t)e * E * E + (size_t)y * E + x];
  const double phi = master[(size_t)env * M * M + layer_phys(y, x, oy, ox, M)];
  corr[(size_t)env * M * M + p] = add_rn(mul_rn(w.x, inv_n), -phi);
  chi[(size_t)env * M * M + p] = mul_rn(w.y, inv_n);
}

// chi_tile[env][p] = (float)(sum_l chi_l at the front's shift / lambda) for every slot of psi_tile's layout: grid (n_ptiles 32 / 256 rounded
// up, Bp envs); the env is uniform over the workgroup (scalar taps), pad pixels and pad envs get zeros
template <int L>
__global__ __launch_bounds__(256) void k_scint_install(SightLayers chi, const int32_t* __restrict__ ap_index, float* __restrict__ chi_tile, int B, int N, int n_ap,
                                                       int n_ptiles, double inv_lambda) {
  const int env = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_ptiles * 32) return;
  float out = 0.f;
  if (env < B && p < n_ap) {
    int oy[L], ox[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      ox[l] = chi.origin[l][2 * env];
      oy[l] = chi.origin[l][2 * env + 1];
    }
    const LayerReader<L, SightLayers> reader(chi, env, N, oy, ox);
    const int flat = ap_index[p], iy = flat / N, ix = flat - iy * N;
    out = (float)mul_rn(reader.at(iy, ix), inv_lambda);
  }
  chi_tile[psi_tile_index(env, p, n_ptiles)] = out;
}

// The receiver.  Geometry and register order are k_pupil_tile.h's: a lane holds 16 pixels of one env (column lane & 31), the two half-waves
// different pixels.  Per pixel: u (revolutions) as k_wavefront_fit forms it, a = exp(chi), (s, c) = sincos(2 pi u); the receive modes'
// values W[p][k] are uniform over a half-wave (broadcast loads of a [n_ptiles 32][4][2] float64 table, zero rows for pads) and every sum
// is float64 on the vector unit.  chi_tile may be null (chi = 0).
template <int A_PAD>
__global__ __launch_bounds__(256) void k_scint_receive(const f16x8* __restrict__ modes16, const f32x4* __restrict__ psi_tile, const f16x8* __restrict__ act16,
                                                       const f32x4* __restrict__ chi_tile, const double2* __restrict__ wmodes, double* __restrict__ slabs,
                                                       int n_ptiles, int n_ap, int Bp) {
  constexpr int NSTEP = A_PAD / 16;
  __shared__ double red[kScintRows * 32];
  double acc[kScintRows];
#pragma unroll
  for (int j = 0; j < kScintRows; ++j) acc[j] = 0.0;
  f16x8 bh[NSTEP], bl[NSTEP];
  const int lane = threadIdx.x & 63, etile = blockIdx.y;
  pupil_tile_loop<NSTEP>(psi_tile, act16, n_ptiles, bh, bl, [&](int t, const f32x4 (&pc)[4]) {
    f32x4 cx[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) cx[g] = chi_tile ? chi_tile[(((size_t)etile * n_ptiles + t) * 4 + g) * 64 + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x16 d = pupil_phase_mfma<NSTEP>(modes16, t, bh, bl);
    const int left = pupil_left(n_ap, t), h = pupil_half();
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (8 * g + r >= left) continue;   // a pad pixel of the last tile adds nothing
        const float u = fmaf(d[4 * g + r], kPhaseUnscale, pc[g][r]);
        float s, c;
        sincos_rev<0>(u, s, c);
        const double x = (double)cx[g][r], a = (double)expf(cx[g][r]);
        const double er = a * (double)c, ei = a * (double)s;
        const double2* w = wmodes + (size_t)(t * 32 + 8 * g + 4 * h + r) * kScintFiber;
#pragma unroll
        for (int k = 0; k < kScintFiber; ++k) {
          const double2 wk = w[k];
          acc[2 * k] += wk.x * er - wk.y * ei;
          acc[2 * k + 1] += wk.x * ei + wk.y * er;
        }
        acc[2 * kScintFiber] += er;
        acc[2 * kScintFiber + 1] += ei;
        acc[2 * kScintFiber + 2] += a;
        acc[2 * kScintFiber + 3] = fma(a, a, acc[2 * kScintFiber + 3]);
        acc[2 * kScintFiber + 4] += x;
        acc[2 * kScintFiber + 5] = fma(x, x, acc[2 * kScintFiber + 5]);
      }
  });
  // the two half-waves hold different pixels of the same env
#pragma unroll
  for (int j = 0; j < kScintRows; ++j) acc[j] += __shfl_down(acc[j], 32, 64);
  pupil_reduce_store<kScintRows>(red, slabs, Bp, [&](auto put) __attribute__((always_inline)) {
    if (pupil_half() != 0) return;
#pragma unroll
    for (int j = 0; j < kScintRows; ++j) put(j, acc[j]);
  });
}

// one thread per env: the slabs in chunk order, then the four outputs (each nullable)
__global__ __launch_bounds__(256) void k_scint_finish(const double* __restrict__ slabs, int n_chunks, int Bp, int B, int n_ap, double* __restrict__ power,
                                                      double* __restrict__ irradiance, double* __restrict__ strehl, double* __restrict__ sigma_chi2) {
#pragma clang fp contract(off)
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= B) return;
  double T[kScintRows];
  for (int j = 0; j < kScintRows; ++j) T[j] = pupil_slab_sum(slabs, n_chunks, (size_t)kScintRows * Bp, j, Bp, env);
  const double n = (double)n_ap;
  if (power) {
    double pw = 0;
    for (int k = 0; k < kScintFiber; ++k) pw += T[2 * k] * T[2 * k] + T[2 * k + 1] * T[2 * k + 1];
    power[env] = pw;
  }
  const double* S = T + 2 * kScintFiber;
  if (irradiance) irradiance[env] = S[3] / n;
  if (strehl) strehl[env] = (S[0] * S[0] + S[1] * S[1]) / (S[2] * S[2]);
  if (sigma_chi2) {
    const double mean = S[4] / n;
    sigma_chi2[env] = fmax(0.0, S[5] / n - mean * mean);
  }
}

}  // namespace aog
