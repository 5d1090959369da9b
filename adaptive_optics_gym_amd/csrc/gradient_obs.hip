// K14 on the separable observation route (aog_upload_gradient_obs; grad_obs_part for aog_output_gradient).  A translation unit of its own:
// the kernels a step launches and those of gradient.hip keep their code objects as they are.
#include "host_common.h"
#include "k_gradient_obs.h"

using namespace aog_host;

namespace {

// K11's geometry (focal.hip)
int gobs_nxp(const aog_env* e) { return round_up(e->cfg.n_pupil, 32); }
int gobs_nyp(const aog_env* e) { return round_up(e->cfg.n_pupil, 16); }

}  // namespace

namespace aog_host {

void launch_grad_obs_backward(aog_env* e, hipStream_t s, const float* qgrid, size_t grid_env, int Nxp, int env0, int n, double* slabs) {
  with_apad(e->A_pad, [&](auto apad) {
    hipLaunchKernelGGL((aog::k_grad_obs_backward<apad()>), dim3(aog::pupil_chunks(e->n_ptiles), (n + 31) / 32), dim3(256), 0, s, qgrid, e->focal_ap_yx,
                       reinterpret_cast<const aog::f16x8*>(e->grad_mtab16), slabs + env0, grid_env, Nxp, n, e->n_ptiles, e->n_ap, e->Bp);
  });
}

int grad_obs_part(aog_env* e, hipStream_t s, const double* g_obs, double* values) {
  const int N = e->cfg.n_pupil, o = e->cfg.obs_dim, n_obs = e->n_obs;
  int rc;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    // validation form: K11's float64 products for F, then H = m1' (W m2') the same way and q on the aperture pixels
    if (g_obs && !e->gobs_slabs && (rc = dev_alloc(e, &e->gobs_slabs, (size_t)e->A * e->Bp, false)) != AOG_OK) return rc;
    for (int env = 0; env < e->B; ++env) {
      launch_focal_field(e, s, e->obs_E, env);
      launch_cgemm64(s, e->obs_m1d, e->obs_E, e->obs_T, nullptr, o, N, N);
      launch_cgemm64(s, e->obs_T, e->obs_m2d, e->gobs_F, nullptr, o, N, o);
      hipLaunchKernelGGL(aog::k_grad_obs_w64, dim3((n_obs + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(e->gobs_F), n_obs,
                         g_obs ? g_obs + (size_t)env * n_obs : nullptr, values ? values + (size_t)env * (n_obs + 2) : nullptr,
                         reinterpret_cast<double2*>(e->gobs_W));
      if (!g_obs) continue;
      launch_cgemm64(s, e->gobs_m1td, e->gobs_W, e->gobs_P, nullptr, N, o, o);
      launch_cgemm64(s, e->gobs_P, e->gobs_m2td, e->gobs_H, nullptr, N, o, N);
      hipLaunchKernelGGL(aog::k_grad_obs_q64, dim3(1), dim3(256), 0, s, reinterpret_cast<const double2*>(e->obs_E),
                         reinterpret_cast<const double2*>(e->gobs_H), e->ap_index, e->modes64, e->gobs_q, e->gobs_slabs, e->n_ap, e->A, e->Bp, env);
    }
    HIP_TRY(hipGetLastError());
    return AOG_OK;
  }
  const int Nxp = gobs_nxp(e), Nyp = gobs_nyp(e), nxt = Nxp / 32, nyt = (Nyp + 31) / 32, n_chunks = aog::pupil_chunks(e->n_ptiles);
  const size_t grid_env = (size_t)Nyp * Nxp;
  // work buffers of the call's own, on first use (never initialised: every element that is read is written by the call first)
  if (g_obs) {
    if (!e->gobs_wop && (rc = dev_alloc(e, &e->gobs_wop, (size_t)e->gobs_chunk * aog::kGradObsWop * 8, false)) != AOG_OK) return rc;
    if (!e->gobs_wscale && (rc = dev_alloc(e, &e->gobs_wscale, (size_t)e->B, false)) != AOG_OK) return rc;
    if (!e->gobs_slabs && (rc = dev_alloc(e, &e->gobs_slabs, (size_t)n_chunks * e->A_pad * e->Bp, false)) != AOG_OK) return rc;
  }
  for (int env0 = 0; env0 < e->B; env0 += e->gobs_chunk) {
    const int n = std::min(e->gobs_chunk, e->B - env0), n_et = (n + 31) / 32;
    launch_phase_grid(e, s, e->grad_act16, e->gobs_act_ll, e->obs_work.grid, grid_env, Nxp, env0 / 32, n_et);
    launch_obs_pass1(e, s, n);
    hipLaunchKernelGGL(aog::k_grad_obs_field, dim3((n + 3) / 4), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->obs_work.T16),
                       reinterpret_cast<const aog::f16x8*>(e->obs_m2s), nxt, n, o, e->obs_unscale, g_obs ? g_obs + (size_t)env0 * n_obs : nullptr,
                       values ? values + (size_t)env0 * (n_obs + 2) : nullptr, e->gobs_wop, g_obs ? e->gobs_wscale + env0 : nullptr);
    if (!g_obs) continue;
    hipLaunchKernelGGL(aog::k_grad_obs_q, dim3((n * nyt * nxt + 3) / 4), dim3(256), 0, s, e->obs_work.grid, reinterpret_cast<const aog::f16x8*>(e->gobs_wop),
                       reinterpret_cast<const aog::f16x8*>(e->gobs_m1t), reinterpret_cast<const aog::f16x8*>(e->gobs_m2t), Nxp, Nyp, n);
    launch_grad_obs_backward(e, s, e->obs_work.grid, grid_env, Nxp, env0, n, e->gobs_slabs);
  }
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // namespace aog_host

extern "C" {

int aog_upload_gradient_obs(aog_env* e, const aog_obs_mft* t) {
  if (!e || !t || !t->m1 || !t->m2) return fail(AOG_ERR_INVALID, "aog_upload_gradient_obs: null argument");
  if (!e->obs_sep)
    return fail(AOG_ERR_STATE, "aog_upload_gradient_obs: the handle was created with cfg.obs_separable = 0 (table route: aog_output_gradient takes g_obs "
                "there already)");
  if (t->o != e->cfg.obs_dim) return fail(AOG_ERR_INVALID, "aog_upload_gradient_obs: o = %d != cfg.obs_dim = %d", t->o, e->cfg.obs_dim);
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_gradient_obs before aog_upload_tables");
  if (!e->obs_ready) return fail(AOG_ERR_STATE, "aog_upload_gradient_obs before aog_upload_obs_mft");
  if (!e->grad_ready) return fail(AOG_ERR_STATE, "aog_upload_gradient_obs before aog_upload_gradient (again after aog_upload_tables)");
  HIP_TRY(hipSetDevice(e->device));
  e->gobs_ready = false;
  const int N = e->cfg.n_pupil, o = e->cfg.obs_dim;
  int rc;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    std::vector<double> m1t((size_t)N * o * 2), m2t((size_t)o * N * 2);
    for (int v = 0; v < o; ++v)
      for (int y = 0; y < N; ++y)
        for (int c = 0; c < 2; ++c) {
          m1t[((size_t)y * o + v) * 2 + c] = t->m1[((size_t)v * N + y) * 2 + c];
          m2t[((size_t)v * N + y) * 2 + c] = t->m2[((size_t)y * o + v) * 2 + c];
        }
    if ((rc = upload(e, &e->gobs_m1td, m1t, true)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->gobs_m2td, m2t, true)) != AOG_OK) return rc;
    if (!e->gobs_F && (rc = dev_alloc(e, &e->gobs_F, (size_t)o * o * 2, false)) != AOG_OK) return rc;
    if (!e->gobs_W && (rc = dev_alloc(e, &e->gobs_W, (size_t)o * o * 2, false)) != AOG_OK) return rc;
    if (!e->gobs_P && (rc = dev_alloc(e, &e->gobs_P, (size_t)N * o * 2, false)) != AOG_OK) return rc;
    if (!e->gobs_H && (rc = dev_alloc(e, &e->gobs_H, (size_t)N * N * 2, false)) != AOG_OK) return rc;
    if (!e->gobs_q && (rc = dev_alloc(e, &e->gobs_q, (size_t)e->n_ap, false)) != AOG_OK) return rc;
    e->gobs_ready = true;
    return AOG_OK;
  }
  // power-of-two scales as mft_operand_tables takes them: the largest component of a table lands in [1/2, 1)
  auto scale_of = [](const double* v, size_t n) {
    double mx = 0.0;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(v[i]));
    return mx > 0.0 && std::isfinite(mx) ? std::ldexp(1.0, -(std::ilogb(mx) + 1)) : 1.0;
  };
  const double s1 = scale_of(t->m1, (size_t)o * N * 2), s2 = scale_of(t->m2, (size_t)o * N * 2);
  auto put = [](std::vector<_Float16>& tab, size_t tile, int lane, int slot, double re, double im) {
    const double c[2] = {re, im};
    for (int q = 0; q < 2; ++q) {
      const _Float16 hi = (_Float16)(float)c[q];   // round to nearest, like the kernels' split8
      tab[((tile * 4 + 2 * q) * 64 + lane) * 8 + slot] = hi;
      tab[((tile * 4 + 2 * q + 1) * 64 + lane) * 8 + slot] = (_Float16)(float)(c[q] - (double)(float)hi);
    }
  };
  const int Nxp = gobs_nxp(e), Nyp = gobs_nyp(e), nxt = Nxp / 32, nyt = (Nyp + 31) / 32;
  // m1t [y tile][step]: lane l = row y = 32 yt + (l & 31), slot j = v = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 8 s + j (the order in which
  // the accumulator registers of Q = W m2' hold v)
  std::vector<_Float16> m1t((size_t)nyt * 2 * 4 * 64 * 8, (_Float16)0.f), m2t((size_t)nxt * 2 * 4 * 64 * 8, (_Float16)0.f);
  for (int yt = 0; yt < nyt; ++yt)
    for (int sidx = 0; sidx < 2; ++sidx)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int r = 8 * sidx + j, v = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), y = 32 * yt + (l & 31);
          if (v < o && y < N) put(m1t, (size_t)yt * 2 + sidx, l, j, t->m1[((size_t)v * N + y) * 2] * s1, t->m1[((size_t)v * N + y) * 2 + 1] * s1);
        }
  // m2t [x tile][step]: lane l = column x = 32 xt + (l & 31), slot j = u = 16 s + 8 (l >> 5) + j
  for (int xt = 0; xt < nxt; ++xt)
    for (int sidx = 0; sidx < 2; ++sidx)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int u = 16 * sidx + 8 * (l >> 5) + j, x = 32 * xt + (l & 31);
          if (u < o && x < N) put(m2t, (size_t)xt * 2 + sidx, l, j, t->m2[((size_t)x * o + u) * 2] * s2, t->m2[((size_t)x * o + u) * 2 + 1] * s2);
        }
  e->gobs_unscale = 1.0 / (s1 * s2);
  if ((rc = upload(e, &e->gobs_m1t, m1t, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->gobs_m2t, m2t, true)) != AOG_OK) return rc;
  if (!e->gobs_act_ll && (rc = dev_alloc(e, &e->gobs_act_ll, (size_t)e->n_etiles * 32 * e->A_pad, true)) != AOG_OK) return rc;
  // whole env tiles per round: what obs_work holds, or fewer (AOG_GRAD_OBS_CHUNK; tests: several rounds at small sizes)
  e->gobs_chunk = e->obs_work.chunk;
  if (const char* v = getenv("AOG_GRAD_OBS_CHUNK")) e->gobs_chunk = std::max(32, std::min(e->gobs_chunk, atoi(v) / 32 * 32));
  if (e->gobs_wop) dev_release(e, &e->gobs_wop);   // (sized by the chunk)
  e->gobs_ready = true;
  return AOG_OK;
}

}  // extern "C"
