// K4: focal-plane field export (aog_focal_image / aog_focal_images); K11: the observation of the separable route (aog_upload_obs_mft, launch_obs).
#include "host_common.h"
#include "k_focal.h"
#include "k_obs.h"

using namespace aog_host;

namespace aog_host {

float mft_operand_tables(const double* m1, const double* m2, int N, int nf, int nfp, int Nxp, int Nyp, std::vector<_Float16>& m1s,
                         std::vector<_Float16>& m2s) {
  // power-of-two scales: the largest component of a table lands in [1/2, 1)
  auto scale_of = [](const double* v, size_t n) {
    double mx = 0.0;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(v[i]));
    return mx > 0.0 ? std::ldexp(1.0, -(std::ilogb(mx) + 1)) : 1.0;
  };
  const double s1 = scale_of(m1, (size_t)nf * N * 2), s2 = scale_of(m2, (size_t)nf * N * 2);
  auto put = [](std::vector<_Float16>& tab, size_t tile, int lane, int slot, double re, double im) {
    const double c[2] = {re, im};
    for (int q = 0; q < 2; ++q) {
      const _Float16 hi = (_Float16)(float)c[q];   // round to nearest, like the kernels' split8
      tab[((tile * 4 + 2 * q) * 64 + lane) * 8 + slot] = hi;
      tab[((tile * 4 + 2 * q + 1) * 64 + lane) * 8 + slot] = (_Float16)(float)(c[q] - (double)(float)hi);
    }
  };
  // m1s [v block][k-step over y]: lane l = column v = 32 vb + (l & 31), slot j = y = 16 ks + 8 (l >> 5) + j
  m1s.assign((size_t)(nfp / 32) * (Nyp / 16) * 4 * 64 * 8, (_Float16)0.f);
  for (int vb = 0; vb < nfp / 32; ++vb)
    for (int ks = 0; ks < Nyp / 16; ++ks)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int v = 32 * vb + (l & 31), y = 16 * ks + 8 * (l >> 5) + j;
          if (v < nf && y < N) put(m1s, (size_t)vb * (Nyp / 16) + ks, l, j, m1[((size_t)v * N + y) * 2] * s1, m1[((size_t)v * N + y) * 2 + 1] * s1);
        }
  // m2s [u block][x tile][s]: lane l = column u = 32 ub + (l & 31), slot j = x = 32 xt + (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 8 s + j
  // (the order in which pass 1's accumulator registers hold x)
  m2s.assign((size_t)(nfp / 32) * (Nxp / 32) * 2 * 4 * 64 * 8, (_Float16)0.f);
  for (int ub = 0; ub < nfp / 32; ++ub)
    for (int xt = 0; xt < Nxp / 32; ++xt)
      for (int s2i = 0; s2i < 2; ++s2i)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int r = 8 * s2i + j, x = 32 * xt + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), u = 32 * ub + (l & 31);
            if (u < nf && x < N)
              put(m2s, ((size_t)ub * (Nxp / 32) + xt) * 2 + s2i, l, j, m2[((size_t)x * nf + u) * 2] * s2, m2[((size_t)x * nf + u) * 2 + 1] * s2);
          }
  return (float)(1.0 / (s1 * s2));
}

int mft_work_alloc(aog_env* e, MftWork* w, size_t grid_env, size_t t16_env, size_t cap_envs, const char* chunk_env) {
  w->chunk = (int)std::min<size_t>((size_t)e->n_etiles * 32, std::max<size_t>(32, cap_envs / 32 * 32));
  if (const char* v = chunk_env ? getenv(chunk_env) : nullptr) w->chunk = std::max(32, std::min(w->chunk, atoi(v) / 32 * 32));
  if (int rc = dev_alloc(e, &w->grid, (size_t)w->chunk * grid_env, false)) return rc;
  if (int rc = dev_alloc(e, &w->T16, (size_t)w->chunk * t16_env, false)) return rc;
  const size_t n_fill = (size_t)w->chunk * grid_env;
  hipLaunchKernelGGL(aog::k_obs_fill, dim3((unsigned)std::min<size_t>((n_fill + 255) / 256, 4096)), dim3(256), 0, nullptr, w->grid, n_fill, aog::kShOutside);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return AOG_OK;
}

void launch_focal_field(aog_env* e, hipStream_t s, double* E, int env, double ratio, const uint8_t* mask, const double* act_src) {
  const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
  hipLaunchKernelGGL(aog::k_focal_field, dim3((e->n_ap + 255) / 256), dim3(256), 0, s, fast ? e->psi_tile : nullptr, fast ? nullptr : e->psi64,
                     e->modes_f32, e->modes64, e->act_rev, act_src ? act_src : e->act_dm, e->ap_index, reinterpret_cast<double2*>(E), env, e->n_ap,
                     e->n_ptiles, e->A, e->A_pad, e->Bp, e->cfg.wavelength_wfs, ratio, mask);
}
void launch_cgemm64(hipStream_t s, const double* a, const double* b, double* out, float* out32, int R, int K, int Cn, const uint8_t* mask, int env) {
  hipLaunchKernelGGL(aog::k_cgemm_small, dim3((R * Cn + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(a),
                     reinterpret_cast<const double2*>(b), reinterpret_cast<double2*>(out), reinterpret_cast<float2*>(out32), R, K, Cn, mask, env);
}

// K11 geometry: x padded to whole 32-column tiles (one wave each), y to whole 16-row k-steps
static int obs_nxp(const aog_env* e) { return round_up(e->cfg.n_pupil, 32); }
static int obs_nyp(const aog_env* e) { return round_up(e->cfg.n_pupil, 16); }

void launch_obs_pass1(aog_env* e, hipStream_t s, int n) {
  const int Nxp = obs_nxp(e), Nyp = obs_nyp(e);
  hipLaunchKernelGGL(aog::k_obs_pass1, dim3((n * (Nxp / 32) + 3) / 4), dim3(256), 0, s, e->obs_work.grid, reinterpret_cast<const aog::f16x8*>(e->obs_m1s),
                     reinterpret_cast<aog::f16x8*>(e->obs_work.T16), Nxp, Nyp, n);
}

int launch_obs(aog_env* e, hipStream_t s, float* obs_raw, uint16_t* obs, const uint8_t* mask) {
  if (!e->obs_sep) return AOG_OK;
  const int N = e->cfg.n_pupil, o = e->cfg.obs_dim, n_obs = e->n_obs;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    // validation form: per env, E on the pupil grid (k_focal_field writes the aperture pixels; the rest of obs_E stays 0), then the two
    // products in float64
    const double2* F = reinterpret_cast<const double2*>(e->obs_F);
    for (int env = 0; env < e->B; ++env) {
      launch_focal_field(e, s, e->obs_E, env);
      launch_cgemm64(s, e->obs_m1d, e->obs_E, e->obs_T, nullptr, o, N, N);
      launch_cgemm64(s, e->obs_T, e->obs_m2d, e->obs_F + (size_t)env * n_obs * 2, nullptr, o, N, o);
    }
    const int n = e->B * n_obs;
    if (e->det_on)
      hipLaunchKernelGGL(aog::k_obs_finish64_det, dim3((n + 255) / 256), dim3(256), 0, s, F, n, n_obs, e->obs_pw, obs_raw, obs, detector_args(e, mask));
    else
      hipLaunchKernelGGL(aog::k_obs_finish64, dim3((n + 255) / 256), dim3(256), 0, s, F, n, e->obs_pw, obs_raw, obs);
    HIP_TRY(hipGetLastError());
    return AOG_OK;
  }
  if (int rc = obs_tiles(e, s)) return rc;
  if (int rc = load_actuators(e, s, {nullptr, e->obs_act16, e->obs_act_ll})) return rc;   // (own copies: act_rev / act16 are not touched)
  const int Nxp = obs_nxp(e), Nyp = obs_nyp(e), nxt = Nxp / 32;
  const size_t grid_env = (size_t)Nyp * Nxp;
  for (int env0 = 0; env0 < e->B; env0 += e->obs_work.chunk) {
    const int n = std::min(e->obs_work.chunk, e->B - env0), n_et = (n + 31) / 32;
    aog_host::launch_phase_grid(e, s, e->obs_act16, e->obs_act_ll, e->obs_work.grid, grid_env, Nxp, env0 / 32, n_et);
    launch_obs_pass1(e, s, n);
    const size_t off = (size_t)env0 * n_obs;
    if (e->det_on)
      hipLaunchKernelGGL(aog::k_obs_pass2_det, dim3((n + 3) / 4), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->obs_work.T16),
                         reinterpret_cast<const aog::f16x8*>(e->obs_m2s), nxt, n, o, e->obs_unscale, e->obs_pw + off, obs_raw ? obs_raw + off : nullptr,
                         obs ? obs + off : nullptr, detector_args(e, mask), env0);
    else
      hipLaunchKernelGGL(aog::k_obs_pass2, dim3((n + 3) / 4), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->obs_work.T16),
                         reinterpret_cast<const aog::f16x8*>(e->obs_m2s), nxt, n, o, e->obs_unscale, e->obs_pw + off, obs_raw ? obs_raw + off : nullptr,
                         obs ? obs + off : nullptr);
  }
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // namespace aog_host

extern "C" {

int aog_upload_obs_mft(aog_env* e, const aog_obs_mft* t) {
  if (!e || !t || !t->m1 || !t->m2) return fail(AOG_ERR_INVALID, "aog_upload_obs_mft: null argument");
  if (!e->obs_sep) return fail(AOG_ERR_STATE, "aog_upload_obs_mft: the handle was created with cfg.obs_separable = 0 (table route)");
  if (t->o != e->cfg.obs_dim) return fail(AOG_ERR_INVALID, "aog_upload_obs_mft: o = %d != cfg.obs_dim = %d", t->o, e->cfg.obs_dim);
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_obs_mft before aog_upload_tables");
  if (e->obs_ready) return fail(AOG_ERR_STATE, "aog_upload_obs_mft: already uploaded for this handle");
  HIP_TRY(hipSetDevice(e->device));
  const int N = e->cfg.n_pupil, o = e->cfg.obs_dim;
  int rc;
  if ((rc = dev_alloc(e, &e->obs_pw, (size_t)e->B * e->n_obs)) != AOG_OK) return rc;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    if ((rc = upload(e, &e->obs_m1d, t->m1, (size_t)o * N * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->obs_m2d, t->m2, (size_t)o * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->obs_E, (size_t)N * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->obs_T, (size_t)o * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->obs_F, (size_t)e->B * e->n_obs * 2)) != AOG_OK) return rc;
    e->obs_ready = true;
    return AOG_OK;
  }
  const int Nxp = obs_nxp(e), Nyp = obs_nyp(e);
  std::vector<_Float16> m1s, m2s;
  e->obs_unscale = mft_operand_tables(t->m1, t->m2, N, o, 32, Nxp, Nyp, m1s, m2s);
  if ((rc = upload(e, &e->obs_m1s, m1s)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->obs_m2s, m2s)) != AOG_OK) return rc;
  // (shared with K4: where each packed aperture pixel lies on the pupil grid)
  if (!e->focal_ap_yx && (rc = upload(e, &e->focal_ap_yx, ap_yx_table(e))) != AOG_OK) return rc;
  // work buffers for whole env tiles, at most ~512 MB together
  const size_t grid_env = (size_t)Nyp * Nxp, t16_env = (size_t)(Nxp / 32) * 2 * 4 * 64 * 8;
  if ((rc = mft_work_alloc(e, &e->obs_work, grid_env, t16_env, ((size_t)512 << 20) / (grid_env * 4 + t16_env * 2), nullptr)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->obs_act16, (size_t)e->n_etiles * 32 * e->A_pad * 2, true)) != AOG_OK) return rc;
  if ((rc = dev_alloc(e, &e->obs_act_ll, (size_t)e->n_etiles * 32 * e->A_pad, true)) != AOG_OK) return rc;
  e->obs_ready = true;
  return AOG_OK;
}

int aog_focal_image(aog_env* e, int env_index, float* field_dev, void* stream) {
  if (!e || !field_dev) return fail(AOG_ERR_INVALID, "aog_focal_image: null argument");
  if (!e->tables_ready || !e->screens_ready) return fail(AOG_ERR_STATE, "aog_focal_image before aog_upload_tables/aog_set_screens");
  if (!e->n_focal) return fail(AOG_ERR_STATE, "aog_focal_image: focal_m1/focal_m2 were not uploaded");
  if (int rc = check_env_range("aog_focal_image", env_index, 1, e->B)) return rc;
  if (int rcp = refuse_pre_evolved(e, "aog_focal_image")) return rcp;
  const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
  if (fast && e->focal_m1s) return aog_focal_images(e, env_index, 1, field_dev, stream);   // the batched matrix-core path
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = e->cfg.n_pupil, nf = e->n_focal;
  HIP_TRY(hipMemsetAsync(e->focal_E, 0, sizeof(double) * 2 * N * N, s));
  launch_focal_field(e, s, e->focal_E, env_index);
  launch_cgemm64(s, e->focal_m1, e->focal_E, e->focal_T, nullptr, nf, N, N);
  launch_cgemm64(s, e->focal_T, e->focal_m2, nullptr, field_dev, nf, N, nf);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_focal_images(aog_env* e, int first, int count, float* field_dev, void* stream) {
  if (!e || !field_dev) return fail(AOG_ERR_INVALID, "aog_focal_images: null argument");
  if (!e->tables_ready || !e->screens_ready) return fail(AOG_ERR_STATE, "aog_focal_images before aog_upload_tables/aog_set_screens");
  if (!e->n_focal) return fail(AOG_ERR_STATE, "aog_focal_images: focal_m1/focal_m2 were not uploaded");
  if (int rc = check_env_range("aog_focal_images", first, count, e->B)) return rc;
  if (e->cfg.precision != AOG_PRECISION_FAST || !e->focal_m1s)
    return fail(AOG_ERR_UNSUPPORTED, "aog_focal_images: fast-precision handles only (use aog_focal_image on a float64 validation handle)");
  if (int rcp = refuse_pre_evolved(e, "aog_focal_images")) return rcp;
  if (count == 0) return AOG_OK;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = e->cfg.n_pupil, nf = e->n_focal;
  int rc;
  const int Nxp = round_up(N, 128), Nyp = round_up(N, 16), nfp = round_up(nf, 128);
  const size_t grid_env = (size_t)Nyp * Nxp, t16_env = (size_t)(Nxp / 32) * (nfp / 32) * 2 * 4 * 64 * 8;
  if (!e->focal_work.grid) {   // work buffers on first use, at most ~256 MB each
    if ((rc = mft_work_alloc(e, &e->focal_work, grid_env, t16_env, ((size_t)256 << 20) / std::max(grid_env * 4, t16_env * 2), "AOG_FOCAL_CHUNK")) != AOG_OK)
      return rc;
    if ((rc = dev_alloc(e, &e->focal_act_ll, (size_t)e->n_etiles * 32 * e->A_pad, true)) != AOG_OK) return rc;
  }
  // psi_tile is always current for quasi_static / semi_dynamic handles; dynamic ones refresh it here when the step kernel does not use it
  if ((rc = ensure_tiles(e, s)) != AOG_OK) return rc;
  if (e->cfg.atm_dynamic && !e->ring_direct && e->kernel != AOG_KERNEL_MFMA && (rc = pack_from_master(e, 0, e->B, s)) != AOG_OK) return rc;
  // u = psi + Mt a with the CURRENT mirror state of every env (act16 is rewritten from act_dm: the VALU step kernel does not keep it)
  if ((rc = load_actuators(e, s, {e->act_rev, e->act16, e->focal_act_ll})) != AOG_OK) return rc;
  for (int env0 = first / 32 * 32; env0 < first + count; env0 += e->focal_work.chunk) {
    const int env1 = std::min(first + count, env0 + e->focal_work.chunk);          // envs [lo, env1) of this chunk are asked for
    const int lo = std::max(first, env0), n_et = (env1 - env0 + 31) / 32;
    aog_host::launch_phase_grid(e, s, e->act16, e->focal_act_ll, e->focal_work.grid, grid_env, Nxp, env0 / 32, n_et);
    const size_t skip = (size_t)(lo - env0);
    hipLaunchKernelGGL(aog::k_focal_pass1, dim3(Nxp / 128, nfp / 128, env1 - lo), dim3(256), 0, s, e->focal_work.grid + skip * grid_env,
                       reinterpret_cast<const aog::f16x8*>(e->focal_m1s), reinterpret_cast<aog::f16x8*>(e->focal_work.T16), Nxp, Nyp, nfp);
    hipLaunchKernelGGL(aog::k_focal_pass2, dim3(nfp / 128, nfp / 128, env1 - lo), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->focal_work.T16),
                       reinterpret_cast<const aog::f16x8*>(e->focal_m2s), reinterpret_cast<float2*>(field_dev) + (size_t)(lo - first) * nf * nf, Nxp, nfp,
                       nf, e->focal_unscale);
    HIP_TRY(hipGetLastError());
  }
  return AOG_OK;
}

}  // extern "C"
