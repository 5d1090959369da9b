// K14: the analytic gradient of observation, power and Strehl (aog_upload_gradient, aog_output_gradient).  A translation unit of its own: the
// kernels a step launches keep their code objects as they are.
#include "host_common.h"
#include "k_gradient.h"

using namespace aog_host;

extern "C" {

int aog_upload_gradient(aog_env* e, const aog_tables* t) {
  if (!e || !t) return fail(AOG_ERR_INVALID, "aog_upload_gradient: null argument");
  if (!t->modes || !t->wfs_tables || !t->sci_tables) return fail(AOG_ERR_INVALID, "aog_upload_gradient: null table pointer");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_gradient before aog_upload_tables");
  if (e->MRW_used + e->MRS_used > aog::kGradMaxTables || e->n_out > aog::kGradMaxOut || e->A > 256)
    return fail(AOG_ERR_UNSUPPORTED, "aog_upload_gradient: built for <= %d tables, <= %d outputs and act_dim <= 256", aog::kGradMaxTables, aog::kGradMaxOut);
  HIP_TRY(hipSetDevice(e->device));
  e->grad_ready = false;
  if (e->cfg.precision == AOG_PRECISION_FP64) {   // (the float64 kernels read modes64 / tabs64)
    e->grad_ready = true;
    return AOG_OK;
  }
  if (e->MRW_used > 32 || e->MRS_used != 1)
    return fail(AOG_ERR_UNSUPPORTED, "aog_upload_gradient: fast handles are built for <= 32 wfs tables and 1 science table");
  const int n_ap = e->n_ap, A = e->A, TW = e->MRW_used, np = e->n_ptiles;
  // one power of two brings the largest table value into [128, 256)
  double big = 0;
  for (size_t i = 0; i < (size_t)TW * n_ap; ++i) big = std::max(big, std::fabs(t->wfs_tables[i]));
  for (int p = 0; p < n_ap; ++p) big = std::max(big, std::fabs(t->sci_tables[p]));
  if (!(big > 0) || !std::isfinite(big)) return fail(AOG_ERR_INVALID, "aog_upload_gradient: the tables are zero or not finite");
  const float tscale = std::ldexp(1.f, 7 - std::ilogb(big));
  e->grad_tscale = tscale;
  int rc;
  // forward: the wfs tables as one block of rows (pack_tab16_rows); the science table in accumulator order: register j of half-wave h
  // holds pixel pupil_acc_row(j, h) of the tile
  const std::vector<_Float16> f16 = pack_tab16_rows(np, n_ap, TW, 1, tscale, [&](int p, int m) { return t->wfs_tables[(size_t)m * n_ap + p]; });
  std::vector<double> st((size_t)np * 32, 0.0);
  for (int pt = 0; pt < np; ++pt)
    for (int h = 0; h < 2; ++h)
      for (int j = 0; j < 16; ++j)
        if (const int p = pt * 32 + aog::pupil_acc_row(j, h); p < n_ap) st[((size_t)pt * 2 + h) * 16 + j] = t->sci_tables[p];
  // backward: A operand of step s, lane (kg, i = pixel of the tile), element el <-> table 16 s + 8 kg + el: the transpose of that role
  std::vector<_Float16> t16(f16.size(), (_Float16)0.f);
  for (int p = 0; p < n_ap; ++p)
    for (int m = 0; m < TW; ++m) {
      _Float16 hi, lo;
      aog::split_f16((float)t->wfs_tables[(size_t)m * n_ap + p] * tscale, hi, lo);
      const int pt = p >> 5, i = p & 31, sidx = m >> 4, kg = (m >> 3) & 1, el = m & 7;
      const size_t base = ((((size_t)pt * 2 + sidx) * 2) * 64 + (kg * 32 + i)) * 8 + el;
      t16[base] = hi;
      t16[base + (size_t)64 * 8] = lo;
    }
  // the modes as table operands: a buffer of the gradient's own, so that the call does not depend on aog_upload_wavefront_fit
  const std::vector<_Float16> m16 = pack_tab16_rows(np, n_ap, A, aog::pupil_blocks(e->A_pad), aog::kModeScale,
                                                    [&](int p, int k) { return t->modes[(size_t)p * A + k]; });
  if ((rc = upload(e, &e->grad_ftab16, f16, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->grad_ttab16, t16, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->grad_mtab16, m16, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->grad_stab, st, true)) != AOG_OK) return rc;
  if (!e->grad_cop16 && (rc = dev_alloc(e, &e->grad_cop16, (size_t)e->n_etiles * 8 * 64 * 8, true)) != AOG_OK) return rc;
  if (!e->grad_csci && (rc = dev_alloc(e, &e->grad_csci, (size_t)e->n_etiles * 32 * 2, true)) != AOG_OK) return rc;
  e->grad_ready = true;
  return AOG_OK;
}

int aog_output_gradient(aog_env* e, const double* g_obs_dev, const double* g_power_dev, const double* g_strehl_dev, const float* action_dev,
                        double* grad_act_dev, double* grad_action_dev, double* values_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_output_gradient: null argument");
  if (!g_obs_dev && !g_power_dev && !g_strehl_dev) return fail(AOG_ERR_INVALID, "aog_output_gradient: every cotangent pointer is null");
  if (!grad_act_dev && !grad_action_dev && !values_dev) return fail(AOG_ERR_INVALID, "aog_output_gradient: every output pointer is null");
  if (grad_action_dev && e->cfg.sh_operation)
    return fail(AOG_ERR_INVALID, "aog_output_gradient: grad_action on an sh_operation handle (its action is the actuators: ask for grad_act)");
  if (grad_action_dev && !action_dev) return fail(AOG_ERR_INVALID, "aog_output_gradient: grad_action needs action_dev");
  if (int rc = instrument_gate(e, "aog_output_gradient", e->grad_ready, "the gradient's tables were", "aog_upload_gradient")) return rc;
  if (g_obs_dev && e->obs_sep && !e->gobs_ready)
    return fail(AOG_ERR_UNSUPPORTED, "aog_output_gradient: g_obs on the separable observation route (cfg.obs_separable = 1: the observation is a "
                "matrix Fourier transform, not a row of wfs_coef); the power and Strehl gradients are available");
  // the observation's part on the separable route (aog_upload_gradient_obs): its values and, with g_obs, its q (gradient_obs.hip)
  const bool obs_part = e->obs_sep && e->gobs_ready && (g_obs_dev || values_dev);
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
  const int n_chunks = fast ? aog::pupil_chunks(e->n_ptiles) : 1, MR = e->MRW_used + e->MRS_used;
  const int frows = fast ? aog::kGradFwdRows : 2 * MR, brows = fast ? e->A_pad : e->A;
  const double ratio = e->cfg.wavelength_wfs / e->cfg.wavelength_sci;
  int rc;
  // work buffers of the call's own, on first use (never initialised: every element that is read is written by the call first)
  if (!e->grad_fslabs && (rc = dev_alloc(e, &e->grad_fslabs, (size_t)n_chunks * frows * e->Bp, false)) != AOG_OK) return rc;
  if (!e->grad_bslabs && (rc = dev_alloc(e, &e->grad_bslabs, (size_t)n_chunks * brows * e->Bp, false)) != AOG_OK) return rc;
  if (!e->grad_cbuf && (rc = dev_alloc(e, &e->grad_cbuf, (size_t)e->B * MR * 2, false)) != AOG_OK) return rc;
  if (!e->grad_cscale && (rc = dev_alloc(e, &e->grad_cscale, (size_t)e->B, false)) != AOG_OK) return rc;
  if (fast) {
    if ((rc = instrument_operands(e, s, obs_part)) != AOG_OK) return rc;   // (the third term: grad_obs_part's phase grid reads it)
    with_apad(e->A_pad, [&](auto apad) {
      hipLaunchKernelGGL((aog::k_grad_forward<apad()>), dim3(n_chunks, e->n_etiles), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->modes16),
                         reinterpret_cast<const aog::f16x8*>(e->grad_ftab16), e->grad_stab, reinterpret_cast<const aog::f32x4*>(e->psi_tile),
                         reinterpret_cast<const aog::f16x8*>(e->inst_act16), e->grad_fslabs, e->n_ptiles, e->n_ap, e->Bp, ratio);
    });
  } else {
    if (!e->grad_trig && (rc = dev_alloc(e, &e->grad_trig, (size_t)e->B * e->n_ap * 4, false)) != AOG_OK) return rc;
    hipLaunchKernelGGL(aog::k_grad_ref_forward, dim3(e->B), dim3(256), 0, s, e->modes64, e->tabs64, e->psi64, e->act_dm, e->grad_trig, e->grad_fslabs,
                       e->n_ap, e->A, e->MRW_used, e->MRS_used, e->Bp, e->cfg.wavelength_wfs, ratio);
  }
  HIP_TRY(hipGetLastError());
  aog::GradCoefArgs c{};
  c.slabs = e->grad_fslabs;
  c.n_chunks = n_chunks;
  c.rows = frows;
  c.Bp = e->Bp;
  c.TW = fast ? 32 : e->MRW_used;
  c.TS = e->MRS_used;
  c.MRW = e->MRW_used;
  c.MRS = e->MRS_used;
  c.n_obs_tab = e->n_obs_tab;
  c.n_out = e->n_out;
  c.n_obs = e->n_obs;
  c.wfs_coef = e->wfs_coef;
  c.sci_coef = e->sci_coef;
  c.inv_tscale = fast ? 1.0 / (double)e->grad_tscale : 1.0;
  c.g_obs = g_obs_dev;
  c.g_power = g_power_dev;
  c.g_strehl = g_strehl_dev;
  c.values = values_dev;
  c.cbuf = e->grad_cbuf;
  c.cscale = e->grad_cscale;
  c.cop16 = fast ? e->grad_cop16 : nullptr;
  c.csci = fast ? e->grad_csci : nullptr;
  hipLaunchKernelGGL(aog::k_grad_coef, dim3(e->B), dim3(256), 0, s, c);
  HIP_TRY(hipGetLastError());
  if (obs_part && (rc = grad_obs_part(e, s, g_obs_dev, values_dev)) != AOG_OK) return rc;   // (behind k_grad_coef: the observation slots of values)
  if (!grad_act_dev && !grad_action_dev) return AOG_OK;   // (the values alone)
  if (fast) {
    with_apad(e->A_pad, [&](auto apad) {
      hipLaunchKernelGGL((aog::k_grad_backward<apad()>), dim3(n_chunks, e->n_etiles), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->modes16),
                         reinterpret_cast<const aog::f16x8*>(e->grad_ttab16), e->grad_stab, reinterpret_cast<const aog::f16x8*>(e->grad_mtab16),
                         reinterpret_cast<const aog::f32x4*>(e->psi_tile), reinterpret_cast<const aog::f16x8*>(e->inst_act16),
                         reinterpret_cast<const aog::f16x8*>(e->grad_cop16), e->grad_csci, e->grad_bslabs, e->n_ptiles, e->n_ap, e->Bp, ratio,
                         e->grad_tscale);
    });
  } else {
    hipLaunchKernelGGL(aog::k_grad_ref_backward, dim3(e->B), dim3(256), 0, s, e->modes64, e->tabs64, e->grad_cbuf, e->grad_trig, e->grad_bslabs, e->n_ap,
                       e->A, e->MRW_used, e->MRS_used, e->Bp, ratio);
  }
  HIP_TRY(hipGetLastError());
  aog::GradFinishArgs f{};
  f.slabs = e->grad_bslabs;
  f.cscale = e->grad_cscale;
  f.gram = e->gram;
  f.action = action_dev;
  f.grad_act = grad_act_dev;
  f.grad_action = grad_action_dev;
  f.n_chunks = n_chunks;
  f.rows = brows;
  f.Bp = e->Bp;
  f.A = e->A;
  f.factor = 4.0 * M_PI / e->cfg.wavelength_wfs;
  if (fast) f.factor /= (double)aog::kModeScale * (double)e->grad_tscale * (double)aog::kGradQScale;
  f.target = e->cfg.surface_rms_target;
  if (obs_part && g_obs_dev) {
    // the slabs of the observation's q: wscale and the operand scales of m1' m2' (fast); the 2 of q = 2 Re(..) is applied here
    f.slabs2 = e->gobs_slabs;
    f.cscale2 = fast ? e->gobs_wscale : nullptr;
    f.n_chunks2 = n_chunks;
    f.rows2 = brows;
    f.factor2 = 4.0 * M_PI / e->cfg.wavelength_wfs;
    if (fast) f.factor2 *= 2.0 * e->gobs_unscale / (double)aog::kModeScale;
  }
  hipLaunchKernelGGL(aog::k_grad_finish, dim3(e->B), dim3(256), 0, s, f);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
