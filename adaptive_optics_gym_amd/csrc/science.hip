// K13: the science camera (aog_upload_science, aog_science_integrate, aog_science_clear, aog_science_read).  A translation unit of its
// own: the kernels a step launches keep their code objects as they are.
#include "mft_host.h"
#include "k_science.h"

using namespace aog_host;

namespace {

constexpr int kScienceMaxRadii = 32, kScienceMaxWindow = 4096;

MftGeom sci_geom(const aog_env* e) { return mft_geom_wide(e->cfg.n_pupil, e->sci_w); }

void release_science(aog_env* e) {
  e->sci_ready = false;
  dev_release(e, &e->sci_m1s);
  dev_release(e, &e->sci_m2s);
  dev_release(e, &e->sci_work.grid);   // (focal_ap_yx stays: K4 and K11 use it too)
  dev_release(e, &e->sci_work.T16);
  dev_release(e, &e->sci_m1d);
  dev_release(e, &e->sci_m2d);
  dev_release(e, &e->sci_E);
  dev_release(e, &e->sci_T);
  dev_release(e, &e->sci_F);
  dev_release(e, &e->sci_bin);
  dev_release(e, &e->sci_exposure);
  dev_release(e, &e->sci_frames);
}

// the checks every call on an uploaded camera shares (aog_focal_images' preconditions)
int science_ready(aog_env* e, const char* who) {
  return instrument_gate(e, who, e->sci_ready, "the science camera was", "aog_upload_science");
}

}  // namespace

extern "C" {

int aog_upload_science(aog_env* e, const double* m1_host, const double* m2_host, int window, double phase_ratio, double peak_fraction,
                       const int32_t* ee_bin_host, int n_ee) {
  if (!e || !m1_host || !m2_host || !ee_bin_host) return fail(AOG_ERR_INVALID, "aog_upload_science: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_science before aog_upload_tables");
  // (the focal grid's size 2 q num_airy is not in aog_config: the caller's tables define the grid, BatchedAOEnv holds w to it; the cap
  // here only bounds the exposure's size)
  if (window < 2 || (window & 1) || window > kScienceMaxWindow)
    return fail(AOG_ERR_INVALID, "aog_upload_science: window = %d must be even and in [2, %d]", window, kScienceMaxWindow);
  if (n_ee < 1 || n_ee > kScienceMaxRadii) return fail(AOG_ERR_INVALID, "aog_upload_science: n_ee = %d outside [1, %d]", n_ee, kScienceMaxRadii);
  if (!(phase_ratio > 0.0) || !(peak_fraction > 0.0)) return fail(AOG_ERR_INVALID, "aog_upload_science: phase_ratio and peak_fraction must be positive");
  const int w = window, N = e->cfg.n_pupil;
  for (int i = 0; i < w * w; ++i)
    if (ee_bin_host[i] < -1 || ee_bin_host[i] >= n_ee) return fail(AOG_ERR_INVALID, "aog_upload_science: ee_bin[%d] = %d outside [-1, %d)", i, ee_bin_host[i], n_ee);
  if (int rc = refuse_pre_evolved(e, "aog_upload_science")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // (a camera uploaded before may still be integrating into the buffers given back here)
  release_science(e);
  e->sci_w = w;
  e->sci_n_ee = n_ee;
  e->sci_ratio = phase_ratio;
  e->sci_peak = peak_fraction;
  int rc;
  if ((rc = upload(e, &e->sci_bin, ee_bin_host, (size_t)w * w)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->sci_exposure, (size_t)e->B * w * w, true)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->sci_frames, (size_t)e->B, true)) != AOG_OK) return rc;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    if ((rc = upload(e, &e->sci_m1d, m1_host, (size_t)w * N * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->sci_m2d, m2_host, (size_t)w * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->sci_E, (size_t)N * N * 2, true)) != AOG_OK) return rc;   // (zero outside the aperture, for good)
    if ((rc = dev_alloc(e, &e->sci_T, (size_t)w * N * 2, false)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->sci_F, (size_t)w * w * 2, false)) != AOG_OK) return rc;
    e->sci_ready = true;
    return AOG_OK;
  }
  const MftGeom g = sci_geom(e);
  std::vector<_Float16> m1s, m2s;
  e->sci_unscale = mft_operand_tables(m1_host, m2_host, N, w, g, m1s, m2s);
  if ((rc = upload(e, &e->sci_m1s, m1s)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->sci_m2s, m2s)) != AOG_OK) return rc;
  // (shared with K4 and K11; written again in place, since aog_upload_tables may have changed the aperture since it was made)
  if ((rc = upload(e, &e->focal_ap_yx, ap_yx_table(e), true)) != AOG_OK) return rc;
  // work buffers as K4's, at most ~256 MB each
  const size_t grid_env = g.grid_env(), t16_env = g.t16_env();
  if ((rc = mft_work_alloc(e, &e->sci_work, grid_env, t16_env, ((size_t)256 << 20) / std::max(grid_env * 4, t16_env * 2), "AOG_SCIENCE_CHUNK")) != AOG_OK)
    return rc;
  e->sci_ready = true;
  return AOG_OK;
}

int aog_science_integrate(aog_env* e, const uint8_t* mask_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_science_integrate: null argument");
  if (int rc = science_ready(e, "aog_science_integrate")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int w = e->sci_w, w2 = w * w;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    for (int env = 0; env < e->B; ++env) {
      launch_mft64(e, s, {e->sci_m1d, e->sci_m2d, e->sci_E, e->sci_T, w}, e->sci_F, nullptr, env, true, e->sci_ratio, mask_dev);
      hipLaunchKernelGGL(aog::k_science_accum64, dim3((w2 + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(e->sci_F), e->sci_exposure,
                         e->sci_frames, w2, env, mask_dev);
    }
    HIP_TRY(hipGetLastError());
    return AOG_OK;
  }
  int rc;
  if ((rc = instrument_operands(e, s, true)) != AOG_OK) return rc;
  const MftGeom g = sci_geom(e);
  const int Nxp = g.Nxp, Nyp = g.Nyp, nvb = g.nvb, nwg = (nvb + 3) / 4;
  // windows of at most two 32-column blocks: the four waves of a workgroup share the two blocks (k_science_pass1); AOG_SCIENCE_SPLIT=0
  // keeps the one-block-per-wave form with idle waves (same bits; tests and measurements)
  int split = nvb <= 2;
  if (const char* v = getenv("AOG_SCIENCE_SPLIT")) split = split && atoi(v) != 0;
  const size_t grid_env = g.grid_env();
  for (int env0 = 0; env0 < e->B; env0 += e->sci_work.chunk) {
    const int n = std::min(e->sci_work.chunk, e->B - env0), n_et = (n + 31) / 32;
    const int etile0 = env0 / 32;
    with_apad(e->A_pad, [&](auto apad) {
      constexpr int NSTEP = apad() / 16;
      hipLaunchKernelGGL((aog::k_science_phase<apad()>), dim3((e->n_ptiles + 3) / 4, n_et), dim3(256), 0, s, f16x8p(e->modes16),
                         reinterpret_cast<const aog::f32x4*>(e->psi_tile) + (size_t)etile0 * e->n_ptiles * 4 * 64,
                         f16x8p(e->inst_act16) + (size_t)etile0 * NSTEP * 2 * 64,
                         f16x8p(e->inst_act_ll) + (size_t)etile0 * NSTEP * 64, e->focal_ap_yx, e->sci_work.grid, grid_env, Nxp,
                         e->n_ptiles, n_et, e->n_ap, e->B - etile0 * 32, e->sci_ratio, mask_dev ? mask_dev + (size_t)etile0 * 32 : nullptr);
    });
    hipLaunchKernelGGL(aog::k_science_pass1, dim3(Nxp / 128, nwg, n), dim3(256), 0, s, e->sci_work.grid, f16x8p(e->sci_m1s), f16x8p(e->sci_work.T16), Nxp,
                       Nyp, nvb, mask_dev, env0, split);
    hipLaunchKernelGGL(aog::k_science_pass2, dim3(nwg, nwg, n), dim3(256), 0, s, f16x8p(e->sci_work.T16), f16x8p(e->sci_m2s), e->sci_exposure, e->sci_frames,
                       Nxp, nvb, w, e->sci_unscale, mask_dev, env0, split);
    HIP_TRY(hipGetLastError());
  }
  return AOG_OK;
}

int aog_science_clear(aog_env* e, const uint8_t* mask_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_science_clear: null argument");
  if (int rc = science_ready(e, "aog_science_clear")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const int w2 = e->sci_w * e->sci_w;
  hipLaunchKernelGGL(aog::k_science_clear, dim3(std::min((w2 + 255) / 256, 64), e->B), dim3(256), 0, static_cast<hipStream_t>(stream), e->sci_exposure,
                     e->sci_frames, mask_dev, w2);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_science_read(aog_env* e, int first, int count, double* psf_dev, double* strehl_dev, double* ee_dev, int32_t* frames_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_science_read: null argument");
  if (!psf_dev && !strehl_dev && !ee_dev && !frames_dev) return fail(AOG_ERR_INVALID, "aog_science_read: every output pointer is null");
  if (int rc = science_ready(e, "aog_science_read")) return rc;
  if (int rc = check_env_range("aog_science_read", first, count, e->B)) return rc;
  if (count == 0) return AOG_OK;
  HIP_TRY(hipSetDevice(e->device));
  aog::ScienceFinishArgs p{};
  p.exposure = e->sci_exposure;
  p.frames = e->sci_frames;
  p.bin = e->sci_bin;
  p.psf = psf_dev;
  p.strehl = strehl_dev;
  p.ee = ee_dev;
  p.frames_out = frames_dev;
  p.first = first;
  p.w = e->sci_w;
  p.n_ee = e->sci_n_ee;
  p.peak_fraction = e->sci_peak;
  hipLaunchKernelGGL(aog::k_science_finish, dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
