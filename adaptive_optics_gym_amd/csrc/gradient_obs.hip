// K14 on the separable observation route (aog_upload_gradient_obs; grad_obs_part for aog_output_gradient).  A translation unit of its own:
// the kernels a step launches and those of gradient.hip keep their code objects as they are.
#include "mft_host.h"
#include "k_gradient_obs.h"

using namespace aog_host;

namespace aog_host {

void launch_grad_obs_backward(aog_env* e, hipStream_t s, const float* qgrid, size_t grid_env, int Nxp, int env0, int n, double* slabs) {
  with_apad(e->A_pad, [&](auto apad) {
    hipLaunchKernelGGL((aog::k_grad_obs_backward<apad()>), dim3(aog::pupil_chunks(e->n_ptiles), (n + 31) / 32), dim3(256), 0, s, qgrid, e->focal_ap_yx,
                       f16x8p(e->grad_mtab16), slabs + env0, grid_env, Nxp, n, e->n_ptiles, e->n_ap, e->Bp);
  });
}

int grad_obs_part(aog_env* e, hipStream_t s, const double* g_obs, double* values) {
  const int N = e->cfg.n_pupil, o = e->cfg.obs_dim, n_obs = e->n_obs;
  int rc;
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    // validation form: K11's float64 products for F, then H = m1' (W m2') the same way and q on the aperture pixels
    if (g_obs && (rc = need(e, &e->gobs_slabs, (size_t)e->A * e->Bp)) != AOG_OK) return rc;
    for (int env = 0; env < e->B; ++env) {
      launch_mft64(e, s, {e->obs_m1d, e->obs_m2d, e->obs_E, e->obs_T, o}, e->gobs_F, nullptr, env);
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
  const MftGeom g = mft_geom_narrow(N);
  const int Nxp = g.Nxp, Nyp = g.Nyp, nxt = Nxp / 32, nyt = blocks32(Nyp), n_chunks = aog::pupil_chunks(e->n_ptiles);
  const size_t grid_env = g.grid_env();
  // work buffers of the call's own, on first use (never initialised: every element that is read is written by the call first)
  if (g_obs) {
    if ((rc = need(e, &e->gobs_wop, (size_t)e->gobs_chunk * aog::kGradObsWop * 8)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_wscale, (size_t)e->B)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_slabs, (size_t)n_chunks * e->A_pad * e->Bp)) != AOG_OK) return rc;
  }
  for (int env0 = 0; env0 < e->B; env0 += e->gobs_chunk) {
    const int n = std::min(e->gobs_chunk, e->B - env0), n_et = (n + 31) / 32;
    launch_phase_grid(e, s, e->inst_act16, e->inst_act_ll, e->obs_work.grid, grid_env, Nxp, env0 / 32, n_et);
    launch_obs_pass1(e, s, n);
    hipLaunchKernelGGL(aog::k_grad_obs_field, dim3((n + 3) / 4), dim3(256), 0, s, f16x8p(e->obs_work.T16), f16x8p(e->obs_m2s), nxt, n, o, e->obs_unscale,
                       g_obs ? g_obs + (size_t)env0 * n_obs : nullptr,
                       values ? values + (size_t)env0 * (n_obs + 2) : nullptr, e->gobs_wop, g_obs ? e->gobs_wscale + env0 : nullptr);
    if (!g_obs) continue;
    hipLaunchKernelGGL(aog::k_grad_obs_q, dim3((n * nyt * nxt + 3) / 4), dim3(256), 0, s, e->obs_work.grid, f16x8p(e->gobs_wop), f16x8p(e->gobs_m1t),
                       f16x8p(e->gobs_m2t), Nxp, Nyp, n);
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
    if ((rc = need(e, &e->gobs_F, (size_t)o * o * 2)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_W, (size_t)o * o * 2)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_P, (size_t)N * o * 2)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_H, (size_t)N * N * 2)) != AOG_OK) return rc;
    if ((rc = need(e, &e->gobs_q, (size_t)e->n_ap)) != AOG_OK) return rc;
    e->gobs_ready = true;
    return AOG_OK;
  }
  // the transposed tables at mft_operand_tables' power-of-two scales: m1' as A operands (row y, K = v in the order in which the accumulator
  // registers of Q = W m2' hold it), m2' as B operands (column x, K = u)
  const double s1 = scale_of(t->m1, (size_t)o * N * 2), s2 = scale_of(t->m2, (size_t)o * N * 2);
  const MftGeom g = mft_geom_narrow(N);
  const int nxt = g.Nxp / 32, nyt = blocks32(g.Nyp);
  std::vector<_Float16> m1t(operand_f16(nyt, 32)), m2t(operand_f16(nxt, 32));
  pack_tiles(m1t.data(), AOG_TILE_ACCUMULATOR, nyt, 32, N, o,
             [&](int y, int v) { return std::complex<double>(t->m1[((size_t)v * N + y) * 2] * s1, t->m1[((size_t)v * N + y) * 2 + 1] * s1); });
  pack_tiles(m2t.data(), AOG_TILE_NATURAL, nxt, 32, N, o,
             [&](int x, int u) { return std::complex<double>(t->m2[((size_t)x * o + u) * 2] * s2, t->m2[((size_t)x * o + u) * 2 + 1] * s2); });
  e->gobs_unscale = 1.0 / (s1 * s2);
  if ((rc = upload(e, &e->gobs_m1t, m1t, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->gobs_m2t, m2t, true)) != AOG_OK) return rc;
  // whole env tiles per round: what obs_work holds, or fewer (AOG_GRAD_OBS_CHUNK; tests: several rounds at small sizes)
  e->gobs_chunk = e->obs_work.chunk;
  if (const char* v = getenv("AOG_GRAD_OBS_CHUNK")) e->gobs_chunk = std::max(32, std::min(e->gobs_chunk, atoi(v) / 32 * 32));
  if (e->gobs_wop) dev_release(e, &e->gobs_wop);   // (sized by the chunk)
  e->gobs_ready = true;
  return AOG_OK;
}

}  // extern "C"
