// K15's gradient (aog_pyramid_gradient).  A translation unit of its own: the kernels a step or a sensor call launches keep their code
// objects as they are.
#include "mft_host.h"
#include "k_pyramid_grad.h"

using namespace aog_host;

namespace {

// the shapes the matrix-core backward passes are built for (fast handles): two 32-blocks along every axis of the window and the detector
constexpr int kPyrGradMaxWq = 32, kPyrGradMaxNs = 64;

// Work buffers of the float64 form, on the first call: the transposed tables (made on the device from the uploaded ones, in stream order)
// and the per-env scratch.
int grad_buffers64(aog_env* e, hipStream_t s) {
  const int N = e->cfg.n_pupil, w = 2 * e->pyr_wq, ns = e->pyr_ns, n_mod = e->pyr_nmod;
  const bool tables = !e->pyg_m1t || !e->pyg_m2t || !e->pyg_b1t || !e->pyg_b2t;
  int rc;
  if ((rc = need(e, &e->pyg_gpix, (size_t)e->B * 4 * ns * ns)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_gscale, (size_t)e->B)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_m1t, (size_t)n_mod * N * w * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_m2t, (size_t)n_mod * w * N * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_b1t, (size_t)w * 2 * ns * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_b2t, (size_t)2 * ns * w * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_W, (size_t)4 * ns * ns * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_Y, (size_t)2 * ns * w * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_V, (size_t)w * w * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_P, (size_t)N * w * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_H, (size_t)N * N * 2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_q, (size_t)e->n_ap)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_slabs, (size_t)e->A * e->Bp)) != AOG_OK) return rc;
  if (!tables) return AOG_OK;
  auto transpose = [s](const double* in, double* out, int batch, int R, int C) {
    hipLaunchKernelGGL(aog::k_pyr_grad_transpose64, dim3((R * C + 255) / 256, batch), dim3(256), 0, s, reinterpret_cast<const double2*>(in),
                       reinterpret_cast<double2*>(out), R, C);
  };
  transpose(e->pyr_m1d, e->pyg_m1t, n_mod, w, N);
  transpose(e->pyr_m2d, e->pyg_m2t, n_mod, N, w);
  transpose(e->pyr_b1d, e->pyg_b1t, 1, 2 * ns, w);   // b1 [2][n_s][w] as one [2 n_s][w] matrix
  transpose(e->pyr_b2d, e->pyg_b2t, 2, w, ns);       // b2 [2][w][n_s], each half on its own
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

// ---- fast handles ----
// the sensor's geometry (pyramid.hip) with the 32-blocks of the detector (nsb), of the padded pupil rows (nyt) and columns (nxt); kw: the
// padded window as a K axis
struct GradGeom : MftGeom {
  int nsb, nyt, nxt, kw;
};
GradGeom grad_geom(const aog_env* e) {
  const MftGeom g = mft_geom_wide(e->cfg.n_pupil, 2 * e->pyr_wq);
  return {g, blocks32(e->pyr_ns), blocks32(g.Nyp), g.Nxp / 32, 32 * g.nvb};
}

// The transposed operand tables, from the uploaded ones (the same split values in another order: nothing is rounded again), and the chunk's
// work buffers.  First call only; blocks for the copies.
int grad_buffers_fast(aog_env* e, bool values_only) {
  const GradGeom g = grad_geom(e);
  const int n_mod = e->pyr_nmod, ns = e->pyr_ns, chunk = e->pyr_work.chunk;
  int rc;
  if ((rc = need(e, &e->pyg_gpix, (size_t)e->B * 4 * ns * ns)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_gscale, (size_t)e->B)) != AOG_OK) return rc;
  if (values_only) return AOG_OK;
  if ((rc = need(e, &e->pyg_qscale, (size_t)e->B)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_vop, (size_t)chunk * operand_f16(g.nvb, g.kw), true)) != AOG_OK) return rc;   // (the pads stay zero)
  if ((rc = need(e, &e->pyg_wscale, (size_t)chunk)) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_qgrid, (size_t)chunk * g.grid_env())) != AOG_OK) return rc;
  if ((rc = need(e, &e->pyg_slabs, (size_t)aog::pupil_chunks(e->n_ptiles) * e->A_pad * e->Bp)) != AOG_OK) return rc;
  if (e->pyg_m1s_t && e->pyg_m2s_t && e->pyg_b1s_t && e->pyg_b2s_t) return AOG_OK;
  // f16 of one modulation point's m1s / m2s and their transposes, and of one half of b1s / b2s (and of their transposes)
  const size_t m1_el = g.m1_f16(), m2_el = g.m2_f16(), m1t_el = operand_f16(g.nyt, g.kw), m2t_el = operand_f16(g.nxt, g.kw), b_el = operand_f16(g.nsb, g.kw);
  std::vector<_Float16> m1s(n_mod * m1_el), m2s(n_mod * m2_el), b1s(2 * b_el), b2s(2 * b_el);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(m1s.data(), e->pyr_m1s, m1s.size() * 2, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m2s.data(), e->pyr_m2s, m2s.size() * 2, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b1s.data(), e->pyr_b1s, b1s.size() * 2, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b2s.data(), e->pyr_b2s, b2s.size() * 2, hipMemcpyDeviceToHost));
  std::vector<_Float16> m1t(n_mod * m1t_el), m2t(n_mod * m2t_el), b1t(2 * b_el), b2t(2 * b_el);
  // m1t (lane y, K = v accumulator) <- m1s (lane v, K = y natural); m2t (lane x, K = u natural) <- m2s (lane u, K = x accumulator)
  for (int j = 0; j < n_mod; ++j) {
    reorder_tiles(m1t.data() + j * m1t_el, AOG_TILE_ACCUMULATOR, g.nyt, g.kw, m1s.data() + j * m1_el, AOG_TILE_NATURAL, g.nvb, g.Nyp);
    reorder_tiles(m2t.data() + j * m2t_el, AOG_TILE_NATURAL, g.nxt, g.kw, m2s.data() + j * m2_el, AOG_TILE_ACCUMULATOR, g.nvb, g.Nxp);
  }
  // b1t (lane v, K = y' accumulator) <- b1s (lane y', K = v accumulator), each half; b2t from b2s the same way, with u for v and x' for y'
  for (int hh = 0; hh < 2; ++hh) {
    reorder_tiles(b1t.data() + hh * b_el, AOG_TILE_ACCUMULATOR, g.nvb, 32 * g.nsb, b1s.data() + hh * b_el, AOG_TILE_ACCUMULATOR, g.nsb, g.kw);
    reorder_tiles(b2t.data() + hh * b_el, AOG_TILE_ACCUMULATOR, g.nvb, 32 * g.nsb, b2s.data() + hh * b_el, AOG_TILE_ACCUMULATOR, g.nsb, g.kw);
  }
  if ((rc = upload(e, &e->pyg_m1s_t, m1t, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyg_m2s_t, m2t, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyg_b1s_t, b1t, true)) != AOG_OK) return rc;
  return upload(e, &e->pyg_b2s_t, b2t, true);
}

template <int NSB, int NVB>
void launch_back(aog_env* e, hipStream_t s, int env0, int n, const uint8_t* mask_dev) {
  hipLaunchKernelGGL((aog::k_pyr_grad_back<NSB, NVB>), dim3(n), dim3(256), 0, s, f16x8p(e->pyr_fop), f16x8p(e->pyr_b1s), f16x8p(e->pyr_b2s),
                     f16x8p(e->pyg_b1s_t), f16x8p(e->pyg_b2s_t), e->pyg_gpix, e->pyg_gscale, e->pyg_vop, e->pyg_wscale, e->pyr_ns, e->pyr_wq,
                     e->pyr_nmod, pyramid_halves(e), e->pyr_back_unscale, mask_dev, env0);
}

// per chunk of whole env tiles: the phase grid once, per modulation point the two forward passes and the two backward kernels, then the
// modes contraction of the chunk's q grid into the slabs
int backward_fast(aog_env* e, hipStream_t s, const uint8_t* mask_dev, const double* act_src) {
  const GradGeom g = grad_geom(e);
  const int Nxp = g.Nxp, Nyp = g.Nyp, nvb = g.nvb, nsb = g.nsb, n_mod = e->pyr_nmod, nku_used = (2 * e->pyr_wq + 15) / 16;
  const size_t m1t_el = operand_f16(g.nyt, g.kw), m2t_el = operand_f16(g.nxt, g.kw);
  if (int rc = pyramid_operands_begin(e, s, act_src)) return rc;
  for (int env0 = 0; env0 < e->B; env0 += e->pyr_work.chunk) {
    const int n = std::min(e->pyr_work.chunk, e->B - env0);
    pyramid_phase_grid(e, s, env0, n);
    for (int j = 0; j < n_mod; ++j) {
      pyramid_forward_point(e, s, j, env0, n, mask_dev);
      if (nsb == 1 && nvb == 1) launch_back<1, 1>(e, s, env0, n, mask_dev);
      else if (nsb == 1) launch_back<1, 2>(e, s, env0, n, mask_dev);
      else if (nvb == 1) launch_back<2, 1>(e, s, env0, n, mask_dev);
      else launch_back<2, 2>(e, s, env0, n, mask_dev);
      hipLaunchKernelGGL(nvb == 1 ? aog::k_pyr_grad_q<1> : aog::k_pyr_grad_q<2>, dim3((n * g.nyt * g.nxt + 3) / 4), dim3(256), 0, s, e->pyr_work.grid,
                         e->pyg_qgrid, f16x8p(e->pyg_vop), f16x8p(e->pyg_m1s_t + j * m1t_el), f16x8p(e->pyg_m2s_t + j * m2t_el), e->pyg_wscale, Nxp, Nyp, n,
                         nku_used, j == 0, mask_dev, env0);
    }
    hipLaunchKernelGGL(aog::k_pyr_grad_qnorm, dim3(n), dim3(256), 0, s, e->pyg_qgrid, e->focal_ap_yx, e->pyg_qscale, g.grid_env(), Nxp, e->n_ap,
                       mask_dev, env0);
    launch_grad_obs_backward(e, s, e->pyg_qgrid, g.grid_env(), Nxp, env0, n, e->pyg_slabs);
    HIP_TRY(hipGetLastError());
  }
  return pyramid_operands_end(e, s);
}

// float64 validation handles: per env and modulation point the forward products of pyramid_accumulate again (G), then the same chain
// backwards with the transposed matrices, q summed over the modulation points, and the modes contraction
void backward64(aog_env* e, hipStream_t s, const uint8_t* mask_dev, const double* act_src) {
  const int N = e->cfg.n_pupil, w = 2 * e->pyr_wq, ns = e->pyr_ns, n_mod = e->pyr_nmod, nG = 4 * ns * ns;
  const size_t m_el = (size_t)w * N * 2, b_el = (size_t)ns * w * 2;
  for (int env = 0; env < e->B; ++env) {
    for (int j = 0; j < n_mod; ++j) {
      launch_pyramid_point64(e, s, j, env, mask_dev, act_src);
      hipLaunchKernelGGL(aog::k_pyr_grad_w64, dim3((nG + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(e->pyr_G), e->pyg_gpix,
                         reinterpret_cast<double2*>(e->pyg_W), ns, n_mod, env, mask_dev);
      // Y_{sy} [n_s][w] = (W_{sy,0} | W_{sy,1}) [n_s][2 n_s] x the stacked b2' [2 n_s][w]; V [w][w] = b1' [w][2 n_s] x (Y_0 ; Y_1) [2 n_s][w]: the
      // halves the tables are zero in add exact zeros
      for (int sy = 0; sy < 2; ++sy)
        launch_cgemm64(s, e->pyg_W + (size_t)sy * ns * 2 * ns * 2, e->pyg_b2t, e->pyg_Y + sy * b_el, nullptr, ns, 2 * ns, w, mask_dev, env);
      launch_cgemm64(s, e->pyg_b1t, e->pyg_Y, e->pyg_V, nullptr, w, 2 * ns, w, mask_dev, env);
      launch_cgemm64(s, e->pyg_m1t + j * m_el, e->pyg_V, e->pyg_P, nullptr, N, w, w, mask_dev, env);
      launch_cgemm64(s, e->pyg_P, e->pyg_m2t + j * m_el, e->pyg_H, nullptr, N, w, N, mask_dev, env);
      hipLaunchKernelGGL(aog::k_pyr_grad_q64, dim3((e->n_ap + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(e->pyr_E),
                         reinterpret_cast<const double2*>(e->pyg_H), e->ap_index, e->pyg_q, e->n_ap, j == 0, env, mask_dev);
    }
    hipLaunchKernelGGL(aog::k_pyr_grad_modes64, dim3(1), dim3(256), 0, s, e->modes64, e->pyg_q, e->pyg_slabs, e->n_ap, e->A, e->Bp, env, mask_dev);
  }
}

}  // namespace

namespace aog_host {

void release_pyramid_gradient(aog_env* e) {
  dev_release(e, &e->pyg_gpix);
  dev_release(e, &e->pyg_m1t);
  dev_release(e, &e->pyg_m2t);
  dev_release(e, &e->pyg_b1t);
  dev_release(e, &e->pyg_b2t);
  dev_release(e, &e->pyg_W);
  dev_release(e, &e->pyg_Y);
  dev_release(e, &e->pyg_V);
  dev_release(e, &e->pyg_P);
  dev_release(e, &e->pyg_H);
  dev_release(e, &e->pyg_q);
  dev_release(e, &e->pyg_slabs);
  dev_release(e, &e->pyg_gscale);
  dev_release(e, &e->pyg_qscale);
  dev_release(e, &e->pyg_m1s_t);
  dev_release(e, &e->pyg_m2s_t);
  dev_release(e, &e->pyg_b1s_t);
  dev_release(e, &e->pyg_b2s_t);
  dev_release(e, &e->pyg_vop);
  dev_release(e, &e->pyg_wscale);
  dev_release(e, &e->pyg_qgrid);
}

}  // namespace aog_host

extern "C" {

int aog_pyramid_gradient(aog_env* e, const uint8_t* mask_dev, const double* g_frames_dev, const double* g_slopes_dev, const double* act_dev,
                         double* grad_dev, double* frames_dev, double* slopes_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_pyramid_gradient: null argument");
  const bool values_only = !grad_dev && !g_frames_dev && !g_slopes_dev && (frames_dev || slopes_dev);
  if (!grad_dev && !values_only) return fail(AOG_ERR_INVALID, "aog_pyramid_gradient: grad_dev is null (allowed only with no cotangent, for the values alone)");
  if (!values_only && !g_frames_dev && !g_slopes_dev) return fail(AOG_ERR_INVALID, "aog_pyramid_gradient: both cotangent pointers are null");
  if (int rc = pyramid_ready(e, "aog_pyramid_gradient")) return rc;
  const bool fast = e->cfg.precision != AOG_PRECISION_FP64;
  if (fast && !values_only) {
    if (e->pyr_wq > kPyrGradMaxWq || e->pyr_ns > kPyrGradMaxNs)
      return fail(AOG_ERR_UNSUPPORTED, "aog_pyramid_gradient: the backward kernels are built for w_q <= %d and n_s <= %d (this handle: N = %d, w_q = %d, "
                  "n_s = %d)", kPyrGradMaxWq, kPyrGradMaxNs, e->cfg.n_pupil, e->pyr_wq, e->pyr_ns);
    if (!e->grad_ready || !e->grad_mtab16)
      return fail(AOG_ERR_STATE, "aog_pyramid_gradient: fast handles contract with the modes operands of aog_upload_gradient (call it first, again "
                  "after aog_upload_tables)");
  }
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if ((rc = fast ? grad_buffers_fast(e, values_only) : grad_buffers64(e, s)) != AOG_OK) return rc;
  // the clean frame: the forward launches of aog_pyramid_frames at the point of evaluation — only where something reads it
  const bool sweep = g_slopes_dev || frames_dev || slopes_dev;
  if (sweep && (rc = pyramid_accumulate(e, s, mask_dev, act_dev)) != AOG_OK) return rc;
  aog::PyrGradCotArgs c{};
  c.acc = sweep ? e->pyr_acc : nullptr;
  c.g_frames = g_frames_dev;
  c.g_slopes = g_slopes_dev;
  c.g_pix = e->pyg_gpix;
  c.gscale = e->pyg_gscale;
  c.frames = frames_dev;
  c.slopes = slopes_dev;
  c.valid = e->pyr_valid;
  c.mask = mask_dev;
  c.ns = e->pyr_ns;
  c.n_valid = e->pyr_nvalid;
  c.n_mod = e->pyr_nmod;
  hipLaunchKernelGGL(aog::k_pyr_grad_cot, dim3(e->B), dim3(256), 0, s, c);
  HIP_TRY(hipGetLastError());
  if (values_only) return AOG_OK;
  aog::PyrGradFinishArgs f{};
  f.slabs = e->pyg_slabs;
  f.grad = grad_dev;
  f.mask = mask_dev;
  f.Bp = e->Bp;
  f.A = e->A;
  f.factor = 4.0 * M_PI / e->cfg.wavelength_wfs;
  if (fast) {
    if ((rc = backward_fast(e, s, mask_dev, act_dev)) != AOG_OK) return rc;
    f.cscale = e->pyg_gscale;
    f.n_chunks = aog::pupil_chunks(e->n_ptiles);
    f.rows = e->A_pad;
    f.cscale2 = e->pyg_qscale;
    // q = 2 Re(..): the 2; the operand scales of m1' m2' (pyr_unscale) and of b1' b2' (pyr_back_unscale carries 1 / 64 for the stored field,
    // which the backward kernels never see); the modes operands' scale.  (The kernels' own powers of two are in gscale and qscale.)
    f.factor *= 2.0 * (double)e->pyr_unscale * (e->pyr_back_unscale * 64.0) / (double)aog::kModeScale;
  } else {
    backward64(e, s, mask_dev, act_dev);
    f.cscale = nullptr;
    f.n_chunks = 1;
    f.rows = e->A;
  }
  hipLaunchKernelGGL(aog::k_pyr_grad_finish, dim3(e->B), dim3(256), 0, s, f);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
