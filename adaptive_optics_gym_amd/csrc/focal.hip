// K4: focal-plane field export (aog_focal_image / aog_focal_images); K11: the observation of the separable route (aog_upload_obs_mft, launch_obs).
#include "mft_host.h"
#include "k_focal.h"
#include "k_obs.h"

using namespace aog_host;

namespace aog_host {

static_assert(kTileF16 == (size_t)aog::kFocalTile * 8, "an operand tile on the host is the kFocalTile f16x8 the kernels step by");

double scale_of(const double* v, size_t n) {
  double mx = 0.0;
  for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(v[i]));
  return mx > 0.0 && std::isfinite(mx) ? std::ldexp(1.0, -(std::ilogb(mx) + 1)) : 1.0;
}

void reorder_tiles(_Float16* dst, int dst_order, int dst_blocks, int dst_k_pad, const _Float16* src, int src_order, int src_blocks, int src_k_pad) {
  pack_tiles(dst, dst_order, dst_blocks, dst_k_pad, src_k_pad, 32 * src_blocks, [&](int i, int k) {
    const _Float16* p = src + tile_offset(src_order, src_k_pad, k, i);
    return TileParts{{p[0], p[kTilePartF16], p[2 * kTilePartF16], p[3 * kTilePartF16]}};
  });
}

float mft_operand_tables(const double* m1, const double* m2, int N, int nf, const MftGeom& g, std::vector<_Float16>& m1s, std::vector<_Float16>& m2s) {
  const double s1 = scale_of(m1, (size_t)nf * N * 2), s2 = scale_of(m2, (size_t)nf * N * 2);
  m1s.resize(g.m1_f16());
  pack_tiles(m1s.data(), AOG_TILE_NATURAL, g.nvb, g.Nyp, nf, N,
             [&](int v, int y) { return std::complex<double>(m1[((size_t)v * N + y) * 2] * s1, m1[((size_t)v * N + y) * 2 + 1] * s1); });
  m2s.resize(g.m2_f16());
  pack_tiles(m2s.data(), AOG_TILE_ACCUMULATOR, g.nvb, g.Nxp, nf, N,
             [&](int u, int x) { return std::complex<double>(m2[((size_t)x * nf + u) * 2] * s2, m2[((size_t)x * nf + u) * 2 + 1] * s2); });
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

void launch_mft64(aog_env* e, hipStream_t s, const Mft64& t, double* F, float* F32, int env, bool field, double ratio, const uint8_t* mask, const double* act_src) {
  const int N = e->cfg.n_pupil;
  if (field) launch_focal_field(e, s, t.E, env, ratio, mask, act_src);
  launch_cgemm64(s, t.m1, t.E, t.T, nullptr, t.w, N, N, mask, env);
  launch_cgemm64(s, t.T, t.m2, F, F32, t.w, N, t.w, mask, env);
}

int alloc_act_operands(aog_env* e, _Float16** act16, _Float16** act_ll) {
  const size_t n = (size_t)e->n_etiles * 32 * e->A_pad;
  if (int rc = act16 ? need(e, act16, 2 * n, true) : AOG_OK) return rc;
  return act_ll ? need(e, act_ll, n, true) : AOG_OK;
}

int instrument_operands(aog_env* e, hipStream_t s, bool want_ll, const double* act_src) {
  if (!e->inst_act16 || (want_ll && !e->inst_act_ll)) {
    if (int rc = alloc_act_operands(e, &e->inst_act16, want_ll ? &e->inst_act_ll : nullptr)) return rc;
    // (zeroed on the null stream, which s may not wait for: dev_alloc_bytes has waited for the fill)
  }
  // psi_tile holding the screens the last step read: always current on quasi_static / semi_dynamic handles; dynamic ones whose step kernel
  // does not write it refresh it from the master screens (psi_tile alone: nothing a step reads is touched, and the int8 extrusion's work
  // ahead stays, because only what the last step left is read); the operands are the call's own copy: act_rev / act16 are not touched
  if (int rc = obs_tiles(e, s)) return rc;
  return load_actuators(e, s, {nullptr, e->inst_act16, want_ll ? e->inst_act_ll : nullptr}, act_src);
}

void launch_obs_pass1(aog_env* e, hipStream_t s, int n) {
  const MftGeom g = mft_geom_narrow(e->cfg.n_pupil);
  hipLaunchKernelGGL(aog::k_obs_pass1, dim3((n * (g.Nxp / 32) + 3) / 4), dim3(256), 0, s, e->obs_work.grid, f16x8p(e->obs_m1s), f16x8p(e->obs_work.T16),
                     g.Nxp, g.Nyp, n);
}

int launch_obs(aog_env* e, hipStream_t s, float* obs_raw, uint16_t* obs, const uint8_t* mask) {
  if (!e->obs_sep) return AOG_OK;
  const int o = e->cfg.obs_dim, n_obs = e->n_obs;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    // validation form: per env, E on the pupil grid (k_focal_field writes the aperture pixels; the rest of obs_E stays 0), then the two
    // products in float64
    const double2* F = reinterpret_cast<const double2*>(e->obs_F);
    for (int env = 0; env < e->B; ++env) launch_mft64(e, s, {e->obs_m1d, e->obs_m2d, e->obs_E, e->obs_T, o}, e->obs_F + (size_t)env * n_obs * 2, nullptr, env);
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
  const MftGeom g = mft_geom_narrow(e->cfg.n_pupil);
  const int nxt = g.Nxp / 32;
  for (int env0 = 0; env0 < e->B; env0 += e->obs_work.chunk) {
    const int n = std::min(e->obs_work.chunk, e->B - env0), n_et = (n + 31) / 32;
    aog_host::launch_phase_grid(e, s, e->obs_act16, e->obs_act_ll, e->obs_work.grid, g.grid_env(), g.Nxp, env0 / 32, n_et);
    launch_obs_pass1(e, s, n);
    const size_t off = (size_t)env0 * n_obs;
    if (e->det_on)
      hipLaunchKernelGGL(aog::k_obs_pass2_det, dim3((n + 3) / 4), dim3(256), 0, s, f16x8p(e->obs_work.T16), f16x8p(e->obs_m2s), nxt, n, o, e->obs_unscale,
                         e->obs_pw + off, obs_raw ? obs_raw + off : nullptr, obs ? obs + off : nullptr, detector_args(e, mask), env0);
    else
      hipLaunchKernelGGL(aog::k_obs_pass2, dim3((n + 3) / 4), dim3(256), 0, s, f16x8p(e->obs_work.T16), f16x8p(e->obs_m2s), nxt, n, o, e->obs_unscale,
                         e->obs_pw + off, obs_raw ? obs_raw + off : nullptr, obs ? obs + off : nullptr);
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
  const MftGeom g = mft_geom_narrow(N);
  std::vector<_Float16> m1s, m2s;
  e->obs_unscale = mft_operand_tables(t->m1, t->m2, N, o, g, m1s, m2s);
  if ((rc = upload(e, &e->obs_m1s, m1s)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->obs_m2s, m2s)) != AOG_OK) return rc;
  // (shared with K4: where each packed aperture pixel lies on the pupil grid)
  if (!e->focal_ap_yx && (rc = upload(e, &e->focal_ap_yx, ap_yx_table(e))) != AOG_OK) return rc;
  // work buffers for whole env tiles, at most ~512 MB together
  const size_t grid_env = g.grid_env(), t16_env = g.t16_env();
  if ((rc = mft_work_alloc(e, &e->obs_work, grid_env, t16_env, ((size_t)512 << 20) / (grid_env * 4 + t16_env * 2), nullptr)) != AOG_OK) return rc;
  if ((rc = alloc_act_operands(e, &e->obs_act16, &e->obs_act_ll)) != AOG_OK) return rc;
  e->obs_ready = true;
  return AOG_OK;
}

static int check_tile_shape(const char* who, int order, int n_blocks, int k_pad) {
  if ((order != AOG_TILE_NATURAL && order != AOG_TILE_ACCUMULATOR) || n_blocks < 1 || k_pad < 16 || k_pad % 16)
    return fail(AOG_ERR_INVALID, "%s: order %d, %d blocks, k_pad = %d (an AOG_TILE_* order, at least one block, k_pad a positive multiple of 16)", who,
                order, n_blocks, k_pad);
  return AOG_OK;
}

int aog_pack_operand_tiles(const double* m, int rows, int K, double scale, int order, int n_blocks, int k_pad, uint16_t* tiles_out) {
  if (!m || !tiles_out || rows < 1 || K < 1) return fail(AOG_ERR_INVALID, "aog_pack_operand_tiles: null argument or empty matrix");
  if (int rc = check_tile_shape("aog_pack_operand_tiles", order, n_blocks, k_pad)) return rc;
  if (rows > 32 * n_blocks || K > k_pad) return fail(AOG_ERR_INVALID, "aog_pack_operand_tiles: [%d][%d] does not fit %d blocks x %d", rows, K, n_blocks, k_pad);
  pack_tiles(reinterpret_cast<_Float16*>(tiles_out), order, n_blocks, k_pad, rows, K,
             [&](int i, int k) { return std::complex<double>(m[((size_t)i * K + k) * 2] * scale, m[((size_t)i * K + k) * 2 + 1] * scale); });
  return AOG_OK;
}

int aog_reorder_operand_tiles(const uint16_t* src, int src_order, int src_blocks, int src_k_pad, int dst_order, int dst_blocks, int dst_k_pad,
                              uint16_t* dst) {
  if (!src || !dst) return fail(AOG_ERR_INVALID, "aog_reorder_operand_tiles: null argument");
  if (int rc = check_tile_shape("aog_reorder_operand_tiles (source)", src_order, src_blocks, src_k_pad)) return rc;
  if (int rc = check_tile_shape("aog_reorder_operand_tiles (destination)", dst_order, dst_blocks, dst_k_pad)) return rc;
  reorder_tiles(reinterpret_cast<_Float16*>(dst), dst_order, dst_blocks, dst_k_pad, reinterpret_cast<const _Float16*>(src), src_order, src_blocks, src_k_pad);
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
  launch_mft64(e, s, {e->focal_m1, e->focal_m2, e->focal_E, e->focal_T, nf}, nullptr, field_dev, env_index);
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
  const MftGeom g = mft_geom_wide(N, round_up(nf, 128));
  const int Nxp = g.Nxp, Nyp = g.Nyp, nfp = 32 * g.nvb;
  const size_t grid_env = g.grid_env(), t16_env = g.t16_env();
  if (!e->focal_work.grid) {   // work buffers on first use, at most ~256 MB each
    if ((rc = mft_work_alloc(e, &e->focal_work, grid_env, t16_env, ((size_t)256 << 20) / std::max(grid_env * 4, t16_env * 2), "AOG_FOCAL_CHUNK")) != AOG_OK)
      return rc;
    if ((rc = alloc_act_operands(e, nullptr, &e->focal_act_ll)) != AOG_OK) return rc;
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
                       f16x8p(e->focal_m1s), f16x8p(e->focal_work.T16), Nxp, Nyp, nfp);
    hipLaunchKernelGGL(aog::k_focal_pass2, dim3(nfp / 128, nfp / 128, env1 - lo), dim3(256), 0, s, f16x8p(e->focal_work.T16), f16x8p(e->focal_m2s),
                       reinterpret_cast<float2*>(field_dev) + (size_t)(lo - first) * nf * nf, Nxp, nfp, nf, e->focal_unscale);
    HIP_TRY(hipGetLastError());
  }
  return AOG_OK;
}

}  // extern "C"
