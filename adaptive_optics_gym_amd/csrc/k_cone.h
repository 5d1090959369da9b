// The layered atmosphere seen from a source at finite range (include/aogym_cone.h): the third Layers type of k_layers.h's passes.  Light
// from a source at range H crosses a layer at altitude h inside a cone, so front pixel (iy, ix) reads source l at the logical position
// (c_l + ctr + m (iy - ctr) + sy, c_l + ctr + m (ix - ctr) + sx), ctr = (N - 1) / 2, m = 1 - h / H in (0, 1]: SightLayers' read with a
// sample position that depends on the pixel.  The position is formed as the sightline's plus a correction, i + floor(s) + q with
// q = (s - floor(s)) + (m - 1)(i - ctr): at m = 1 the correction is an exact zero and every weight and index is SightLayers' own, so an env
// at m = 1 holds the plane-wave installation's bits without a branch.  Per env and source — wave-uniform, scalar loads — a ConeTap holds
// k = m - 1, floor(s) folded with the margin and the ring origin into one offset per axis in [0, N_l), and s - floor(s); the rest is the
// pixel's own: per axis one product, one sum, one floor and two differences in float64, then SightLayers' four loads, four products and
// three sums.  For m <= 1 neighbouring front pixels read the same or neighbouring source pixels, so a wave's gathers stay inside the lines
// the sightline reader touches.
#pragma once
#include "k_layers.h"

namespace aog {

struct LayerCone {
  const double* geom[kMaxLayers];   // [B][3] (sx, sy, m) of this source: pixels, pixels, magnification
  int n[kMaxLayers];                // N_l
  int c[kMaxLayers];                // c_l
};
struct ConeLayers : LayerSources {
  LayerCone cone;
};
struct ConeTap {
  double k, ry, rx;   // m - 1; sy - floor(sy), sx - floor(sx)
  int by, bx;         // (oy + c_l + floor(sy)) mod N_l, (ox + c_l + floor(sx)) mod N_l
};

// One axis of one pixel: d = i - ctr (an exact half-integer), r = s - floor(s).  q = (k d) + r, q0 = floor(q), f = q - q0, g = 1 - f, each
// rounded on its own in that order; the first sample sits i + q0 pixels from the folded origin b.  The host has checked that the sample
// stays inside the margin, so b + i + q0 lies in (-N_l, 2 N_l) and one conditional correction each way brings both samples' ring indices
// into [0, N_l).
__device__ __forceinline__ void cone_axis(int i, double d, double k, double r, int b, int n, int& i0, int& i1, double& g, double& f) {
  const double q = add_rn(mul_rn(k, d), r);
  const double q0 = floor(q);
  f = add_rn(q, -q0);
  g = add_rn(1.0, -f);
  int j = b + i + (int)q0;
  j = j < 0 ? j + n : j;
  j = j >= n ? j - n : j;
  i0 = j;
  i1 = j + 1 == n ? 0 : j + 1;
}

template <int L>
struct LayerReader<L, ConeLayers> {
  static constexpr int kInFlight = 4;   // x 4 L loads
  const ConeLayers& layers;
  const int env;
  const double ctr;
  ConeTap tap[L];
  __device__ __forceinline__ LayerReader(const ConeLayers& layers, int env, int N, const int (&oy)[L], const int (&ox)[L])
      : layers(layers), env(env), ctr(0.5 * (double)(N - 1)) {
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const double* g = layers.cone.geom[l] + 3 * (size_t)env;
      const double x0 = floor(g[0]), y0 = floor(g[1]);
      tap[l].rx = add_rn(g[0], -x0);
      tap[l].ry = add_rn(g[1], -y0);
      tap[l].k = add_rn(g[2], -1.0);
      tap[l].bx = ring_mod(ox[l] + layers.cone.c[l] + (int)x0, layers.cone.n[l]);
      tap[l].by = ring_mod(oy[l] + layers.cone.c[l] + (int)y0, layers.cone.n[l]);
    }
  }
  // s = v_0 + v_1 + ... in source order at front pixel (iy, ix); every address lies inside the env's screen
  __device__ __forceinline__ double at(int iy, int ix) const {
    const double dy = add_rn((double)iy, -ctr), dx = add_rn((double)ix, -ctr);
    double v[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const int n = layers.cone.n[l];
      const double* src = layers.master[l] + (size_t)env * n * n;
      int y0, y1, x0, x1;
      double gy, fy, gx, fx;
      cone_axis(iy, dy, tap[l].k, tap[l].ry, tap[l].by, n, y0, y1, gy, fy);
      cone_axis(ix, dx, tap[l].k, tap[l].rx, tap[l].bx, n, x0, x1, gx, fx);
      const double v00 = src[y0 * n + x0], v01 = src[y0 * n + x1];
      const double v10 = src[y1 * n + x0], v11 = src[y1 * n + x1];
      const double top = add_rn(mul_rn(gx, v00), mul_rn(fx, v01));
      const double bottom = add_rn(mul_rn(gx, v10), mul_rn(fx, v11));
      v[l] = add_rn(mul_rn(gy, top), mul_rn(fy, bottom));
    }
    double s = v[0];
#pragma unroll
    for (int l = 1; l < L; ++l) s = add_rn(s, v[l]);
    return s;
  }
};

}  // namespace aog
