// K15: the modulated pyramid wavefront sensor (aog_upload_pyramid, aog_pyramid_frames, aog_pyramid_slopes, aog_upload_pyramid_reconstructor,
// aog_pyramid_update).  A translation unit of its own: the kernels a step launches keep their code objects as they are.
#include "mft_host.h"
#include "k_pyramid.h"

using namespace aog_host;

namespace {

constexpr int kPyrMinSide = 8, kPyrMaxSide = 64, kPyrMaxMod = 32;
static_assert(sizeof(aog_pyramid_tables) == 4 * 4 + 9 * 8 + 3 * 8, "aog_pyramid_tables: four int32, nine pointers, three doubles, no padding (the ctypes mirror relies on it)");

// the science camera's geometry, for the window of both halves
MftGeom pyr_geom(const aog_env* e) { return mft_geom_wide(e->cfg.n_pupil, 2 * e->pyr_wq); }

void release_pyramid(aog_env* e) {
  e->pyr_ready = e->pyr_rec_ready = false;
  dev_release(e, &e->pyr_m1s);
  dev_release(e, &e->pyr_m2s);
  dev_release(e, &e->pyr_b1s);
  dev_release(e, &e->pyr_b2s);
  dev_release(e, &e->pyr_work.grid);   // (focal_ap_yx stays: K4, K11 and the science camera use it too)
  dev_release(e, &e->pyr_work.T16);
  dev_release(e, &e->pyr_fop);
  dev_release(e, &e->pyr_tile_keep);
  dev_release(e, &e->pyr_m1d);
  dev_release(e, &e->pyr_m2d);
  dev_release(e, &e->pyr_b1d);
  dev_release(e, &e->pyr_b2d);
  dev_release(e, &e->pyr_E);
  dev_release(e, &e->pyr_T);
  dev_release(e, &e->pyr_F);
  dev_release(e, &e->pyr_X);
  dev_release(e, &e->pyr_G);
  dev_release(e, &e->pyr_valid);
  dev_release(e, &e->pyr_acc);
  dev_release(e, &e->pyr_slopes);
  dev_release(e, &e->pyr_recon);
  dev_release(e, &e->pyr_ref);
  release_pyramid_gradient(e);
}

}  // namespace

namespace aog_host {

// the checks every call on an uploaded sensor shares (aog_science_integrate's preconditions)
int pyramid_ready(aog_env* e, const char* who) {
  return instrument_gate(e, who, e->pyr_ready, "the pyramid sensor was", "aog_upload_pyramid");
}

// The sum over the modulation points of every selected env into pyr_acc (no division yet: k_pyr_finish).
int pyramid_accumulate(aog_env* e, hipStream_t s, const uint8_t* mask_dev, const double* act_src) {
  const int ns = e->pyr_ns, n_mod = e->pyr_nmod;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    const int nG = 4 * ns * ns;
    for (int env = 0; env < e->B; ++env)
      for (int j = 0; j < n_mod; ++j) {
        launch_pyramid_point64(e, s, j, env, mask_dev, act_src);
        hipLaunchKernelGGL(aog::k_pyr_accum64, dim3((nG + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(e->pyr_G), e->pyr_acc, nG, env,
                           j == 0, mask_dev);
      }
    HIP_TRY(hipGetLastError());
    return AOG_OK;
  }
  if (int rc = pyramid_operands_begin(e, s, act_src)) return rc;
  const int nsb = blocks32(ns), nvb = pyr_geom(e).nvb;
  // 16-row k-steps of the two halves of the window
  const int4 half = pyramid_halves(e);
  for (int env0 = 0; env0 < e->B; env0 += e->pyr_work.chunk) {
    const int n = std::min(e->pyr_work.chunk, e->B - env0);
    pyramid_phase_grid(e, s, env0, n);   // once: the grid is read n_mod times
    for (int j = 0; j < n_mod; ++j) {
      pyramid_forward_point(e, s, j, env0, n, mask_dev);
      hipLaunchKernelGGL(nsb == 1 ? aog::k_pyr_back<1> : aog::k_pyr_back<2>, dim3(n), dim3(256), 0, s, f16x8p(e->pyr_fop), f16x8p(e->pyr_b1s),
                         f16x8p(e->pyr_b2s), e->pyr_acc, nvb, ns, half, e->pyr_back_unscale, j == 0, mask_dev, env0);
    }
    HIP_TRY(hipGetLastError());
  }
  return pyramid_operands_end(e, s);
}

void launch_pyramid_point64(aog_env* e, hipStream_t s, int j, int env, const uint8_t* mask_dev, const double* act_src) {
  const int N = e->cfg.n_pupil, w = 2 * e->pyr_wq, ns = e->pyr_ns;
  const size_t m_el = (size_t)w * N * 2, b_el = (size_t)ns * w * 2;
  launch_mft64(e, s, {e->pyr_m1d + j * m_el, e->pyr_m2d + j * m_el, e->pyr_E, e->pyr_T, w}, e->pyr_F, nullptr, env, j == 0, 1.0, mask_dev, act_src);
  for (int sy = 0; sy < 2; ++sy) launch_cgemm64(s, e->pyr_b1d + sy * b_el, e->pyr_F, e->pyr_X + sy * b_el, nullptr, ns, w, w, mask_dev, env);
  for (int q = 0; q < 4; ++q)
    launch_cgemm64(s, e->pyr_X + (q >> 1) * b_el, e->pyr_b2d + (q & 1) * b_el, e->pyr_G + (size_t)q * ns * ns * 2, nullptr, ns, w, ns, mask_dev, env);
}

int4 pyramid_halves(const aog_env* e) {
  const int wq = e->pyr_wq, w = 2 * wq;
  return make_int4(0, (wq + 15) / 16, wq / 16, (w + 15) / 16);
}

static bool pyr_keeps_tiles(const aog_env* e) { return e->pyr_tile_keep && e->kernel != AOG_KERNEL_MFMA && !e->sh_ready; }
static size_t pyr_tile_bytes(const aog_env* e) { return sizeof(float) * (size_t)e->n_etiles * e->n_ptiles * 1024; }

int pyramid_operands_begin(aog_env* e, hipStream_t s, const double* act_src) {
  // (a dynamic handle that steps with the VALU kernel keeps a psi_tile nobody reads between its screen installations, but the state blob
  // carries it: the call leaves it as it found it, so that aog_get_state does not depend on whether the sensor was called)
  if (pyr_keeps_tiles(e)) HIP_TRY(hipMemcpyAsync(e->pyr_tile_keep, e->psi_tile, pyr_tile_bytes(e), hipMemcpyDeviceToDevice, s));
  return instrument_operands(e, s, true, act_src);
}

int pyramid_operands_end(aog_env* e, hipStream_t s) {
  if (pyr_keeps_tiles(e)) HIP_TRY(hipMemcpyAsync(e->psi_tile, e->pyr_tile_keep, pyr_tile_bytes(e), hipMemcpyDeviceToDevice, s));
  return AOG_OK;
}

void pyramid_phase_grid(aog_env* e, hipStream_t s, int env0, int n) {
  const MftGeom g = pyr_geom(e);
  launch_phase_grid(e, s, e->inst_act16, e->inst_act_ll, e->pyr_work.grid, g.grid_env(), g.Nxp, env0 / 32, (n + 31) / 32);
}

// F_j of the chunk's envs into pyr_fop: the two forward passes
void pyramid_forward_point(aog_env* e, hipStream_t s, int j, int env0, int n, const uint8_t* mask_dev) {
  const MftGeom g = pyr_geom(e);
  const int Nxp = g.Nxp, nvb = g.nvb, nwg = (nvb + 3) / 4, split = nvb <= 2, w = 2 * e->pyr_wq;
  hipLaunchKernelGGL(aog::k_pyr_pass1, dim3(Nxp / 128, nwg, n), dim3(256), 0, s, e->pyr_work.grid, f16x8p(e->pyr_m1s + j * g.m1_f16()),
                     f16x8p(e->pyr_work.T16), Nxp, g.Nyp, nvb, mask_dev, env0, split);
  hipLaunchKernelGGL(aog::k_pyr_pass2, dim3(nwg, nwg, n), dim3(256), 0, s, f16x8p(e->pyr_work.T16), f16x8p(e->pyr_m2s + j * g.m2_f16()), e->pyr_fop, Nxp,
                     nvb, w, e->pyr_unscale * aog::kPyrFieldScale, mask_dev, env0);
}

}  // namespace aog_host

namespace {

// accumulate + finish: the shared body of the three sensor calls
int pyramid_sense(aog_env* e, hipStream_t s, const uint8_t* mask_dev, double* frames_dev, double* slopes_dev) {
  if (int rc = pyramid_accumulate(e, s, mask_dev)) return rc;
  aog::PyrFinishArgs p{};
  p.acc = e->pyr_acc;
  p.frames = frames_dev;
  p.slopes = slopes_dev;
  p.valid = e->pyr_valid;
  p.mask = mask_dev;
  p.ns = e->pyr_ns;
  p.n_valid = e->pyr_nvalid;
  p.n_mod = e->pyr_nmod;
  p.env_base = e->cfg.env_id_base;
  p.photons = e->pyr_photons;
  p.seed = e->rng_seed;
  p.frame_lo = (uint32_t)e->pyr_frame;
  p.frame_hi = (uint32_t)(e->pyr_frame >> 32);
  hipLaunchKernelGGL(aog::k_pyr_finish, dim3(e->B), dim3(256), 0, s, p);
  HIP_TRY(hipGetLastError());
  ++e->pyr_frame;
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_upload_pyramid(aog_env* e, const aog_pyramid_tables* t) {
  if (!e || !t) return fail(AOG_ERR_INVALID, "aog_upload_pyramid: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_pyramid before aog_upload_tables");
  const bool f64 = e->cfg.precision == AOG_PRECISION_FP64;
  const int N = e->cfg.n_pupil, wq = t->samples, w = 2 * wq, ns = t->pixels, n_mod = t->n_mod, nv = t->n_valid;
  if (wq < kPyrMinSide || wq > kPyrMaxSide) return fail(AOG_ERR_INVALID, "aog_upload_pyramid: samples = %d outside [%d, %d]", wq, kPyrMinSide, kPyrMaxSide);
  if (ns < kPyrMinSide || ns > kPyrMaxSide || ns > N)
    return fail(AOG_ERR_INVALID, "aog_upload_pyramid: pixels = %d outside [%d, min(%d, n_pupil = %d)]", ns, kPyrMinSide, kPyrMaxSide, N);
  if (n_mod < 1 || n_mod > kPyrMaxMod) return fail(AOG_ERR_INVALID, "aog_upload_pyramid: n_mod = %d outside [1, %d]", n_mod, kPyrMaxMod);
  if (nv < 1 || nv > ns * ns || !t->valid) return fail(AOG_ERR_INVALID, "aog_upload_pyramid: n_valid = %d outside [1, %d] (or valid is null)", nv, ns * ns);
  for (int k = 0; k < nv; ++k)
    if (t->valid[k] < 0 || t->valid[k] >= ns * ns || (k && t->valid[k] <= t->valid[k - 1]))
      return fail(AOG_ERR_INVALID, "aog_upload_pyramid: valid[%d] = %d must lie in [0, %d) and ascend", k, t->valid[k], ns * ns);
  if (!(t->photons >= 0.0) || !std::isfinite(t->photons)) return fail(AOG_ERR_INVALID, "aog_upload_pyramid: photons must be finite and >= 0");
  if (f64 ? (!t->m1 || !t->m2 || !t->b1 || !t->b2) : (!t->m1s || !t->m2s || !t->b1s || !t->b2s))
    return fail(AOG_ERR_INVALID, "aog_upload_pyramid: null table (%s)", f64 ? "float64 handles read m1, m2, b1, b2" : "fast handles read m1s, m2s, b1s, b2s");
  auto pow2 = [](double v) { int ex; return v > 0.0 && std::isfinite(v) && std::frexp(v, &ex) == 0.5; };
  if (!f64 && (!pow2(t->fwd_unscale) || !pow2(t->back_unscale)))
    return fail(AOG_ERR_INVALID, "aog_upload_pyramid: fwd_unscale and back_unscale must be powers of two");
  if (int rc = refuse_pre_evolved(e, "aog_upload_pyramid")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // (a sensor uploaded before may still be working in the buffers given back here)
  release_pyramid(e);
  e->pyr_wq = wq;
  e->pyr_ns = ns;
  e->pyr_nmod = n_mod;
  e->pyr_nvalid = nv;
  e->pyr_photons = t->photons;
  e->pyr_frame = 0;
  int rc;
  if ((rc = upload(e, &e->pyr_valid, t->valid, (size_t)nv)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->pyr_acc, (size_t)e->B * 4 * ns * ns, true)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->pyr_slopes, (size_t)e->B * 2 * nv, true)) != AOG_OK) return rc;
  if (f64) {
    if ((rc = upload(e, &e->pyr_m1d, t->m1, (size_t)n_mod * w * N * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->pyr_m2d, t->m2, (size_t)n_mod * w * N * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->pyr_b1d, t->b1, (size_t)2 * ns * w * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->pyr_b2d, t->b2, (size_t)2 * ns * w * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->pyr_E, (size_t)N * N * 2, true)) != AOG_OK) return rc;   // (zero outside the aperture, for good)
    if ((rc = dev_alloc(e, &e->pyr_T, (size_t)w * N * 2, false)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->pyr_F, (size_t)w * w * 2, false)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->pyr_X, (size_t)2 * ns * w * 2, false)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->pyr_G, (size_t)4 * ns * ns * 2, false)) != AOG_OK) return rc;
    e->pyr_ready = true;
    return AOG_OK;
  }
  const MftGeom g = pyr_geom(e);
  const size_t b_el = 2 * operand_f16(blocks32(ns), 32 * g.nvb), fop_env = operand_f16(g.nvb, 32 * g.nvb);   // (both halves' b tables; F_j of one env)
  e->pyr_unscale = (float)t->fwd_unscale;
  e->pyr_back_unscale = t->back_unscale / (double)aog::kPyrFieldScale;
  static_assert(sizeof(_Float16) == sizeof(uint16_t), "the operand tables arrive as IEEE half bits");
  if ((rc = upload(e, &e->pyr_m1s, reinterpret_cast<const _Float16*>(t->m1s), g.m1_f16() * n_mod)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyr_m2s, reinterpret_cast<const _Float16*>(t->m2s), g.m2_f16() * n_mod)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyr_b1s, reinterpret_cast<const _Float16*>(t->b1s), b_el)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyr_b2s, reinterpret_cast<const _Float16*>(t->b2s), b_el)) != AOG_OK) return rc;
  // (shared with K4, K11 and the science camera; written again in place, since aog_upload_tables may have changed the aperture since it was made)
  if ((rc = upload(e, &e->focal_ap_yx, ap_yx_table(e), true)) != AOG_OK) return rc;
  // work buffers as the science camera's, at most ~256 MB each
  const size_t grid_env = g.grid_env(), t16_env = g.t16_env();
  if ((rc = mft_work_alloc(e, &e->pyr_work, grid_env, t16_env, ((size_t)256 << 20) / std::max(grid_env * 4, std::max(t16_env, fop_env) * 2),
                           "AOG_PYRAMID_CHUNK")) != AOG_OK)
    return rc;
  if ((rc = dev_alloc(e, &e->pyr_fop, (size_t)e->pyr_work.chunk * fop_env, true)) != AOG_OK) return rc;   // (the pads stay zero)
  if (e->cfg.atm_dynamic && !e->ring_direct && (rc = dev_alloc(e, &e->pyr_tile_keep, (size_t)e->n_etiles * e->n_ptiles * 1024, false)) != AOG_OK) return rc;
  e->pyr_ready = true;
  return AOG_OK;
}

int aog_pyramid_frames(aog_env* e, const uint8_t* mask_dev, double* frames_dev, void* stream) {
  if (!e || !frames_dev) return fail(AOG_ERR_INVALID, "aog_pyramid_frames: null argument");
  if (int rc = pyramid_ready(e, "aog_pyramid_frames")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return pyramid_sense(e, static_cast<hipStream_t>(stream), mask_dev, frames_dev, nullptr);
}

int aog_pyramid_slopes(aog_env* e, const uint8_t* mask_dev, double* slopes_dev, void* stream) {
  if (!e || !slopes_dev) return fail(AOG_ERR_INVALID, "aog_pyramid_slopes: null argument");
  if (int rc = pyramid_ready(e, "aog_pyramid_slopes")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return pyramid_sense(e, static_cast<hipStream_t>(stream), mask_dev, nullptr, slopes_dev);
}

int aog_upload_pyramid_reconstructor(aog_env* e, const double* recon_host, const double* slopes_ref_host) {
  if (!e || !recon_host || !slopes_ref_host) return fail(AOG_ERR_INVALID, "aog_upload_pyramid_reconstructor: null argument");
  if (!e->pyr_ready) return fail(AOG_ERR_STATE, "aog_upload_pyramid_reconstructor before aog_upload_pyramid");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // (an update may still be reading the tables written again here)
  const size_t n_sl = (size_t)2 * e->pyr_nvalid;
  int rc;
  if ((rc = upload(e, &e->pyr_recon, recon_host, (size_t)e->A * n_sl, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->pyr_ref, slopes_ref_host, n_sl, true)) != AOG_OK) return rc;
  e->pyr_rec_ready = true;
  return AOG_OK;
}

int aog_pyramid_update(aog_env* e, double gain, double* act_out_dev, double* slopes_dev, void* stream) {
  if (!e || !act_out_dev) return fail(AOG_ERR_INVALID, "aog_pyramid_update: null argument");
  if (!std::isfinite(gain)) return fail(AOG_ERR_INVALID, "aog_pyramid_update: gain must be finite");
  if (int rc = pyramid_ready(e, "aog_pyramid_update")) return rc;
  if (!e->pyr_rec_ready) return fail(AOG_ERR_STATE, "aog_pyramid_update before aog_upload_pyramid_reconstructor");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* sl = slopes_dev ? slopes_dev : e->pyr_slopes;
  if (int rc = pyramid_sense(e, s, nullptr, nullptr, sl)) return rc;
  hipLaunchKernelGGL(aog::k_pyr_update, dim3(e->B), dim3(256), 0, s, e->act_dm, sl, e->pyr_recon, e->pyr_ref, act_out_dev, e->A, 2 * e->pyr_nvalid, gain);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
