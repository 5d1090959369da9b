// K10's gradient (aog_sh_gradient).  A translation unit of its own: the kernels aog_sh_image / aog_sh_update launch keep their code objects
// as they are.
#include "mft_host.h"
#include "k_shack_back.h"
#include "../../include/aogym_shack_gradient.h"
#include <hipfft/hipfft.h>

using namespace aog_host;

namespace {

bool separable(const aog_env* e) { return e->sh_pruned && e->sh_sep_rl; }

// Work buffers, on the first call (blocking copies: the lenslets' pixel lists are made on the host from the uploaded slot map)
int grad_buffers(aog_env* e, bool values_only) {
  const int N = e->cfg.n_pupil, B = e->B;
  const size_t N2 = (size_t)N * N;
  int rc;
  if ((rc = need(e, &e->shg_act16, (size_t)e->n_etiles * e->A_pad * 32 * 2, true)) != AOG_OK) return rc;
  if ((rc = need(e, &e->shg_image, (size_t)B * N2)) != AOG_OK) return rc;
  if ((rc = need(e, &e->shg_coef, (size_t)B * e->sh_n_sub * 4, true)) != AOG_OK) return rc;
  if (!e->shg_slot_start) {
    std::vector<int32_t> slot(N2), start((size_t)e->sh_n_sub + 1, 0), pix;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(slot.data(), e->sh_slot, sizeof(int32_t) * N2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N2; ++i)
      if (slot[i] >= 0) ++start[slot[i] + 1];
    for (int s = 0; s < e->sh_n_sub; ++s) start[s + 1] += start[s];
    pix.resize((size_t)start[e->sh_n_sub]);
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for (size_t i = 0; i < N2; ++i)
      if (slot[i] >= 0) pix[(size_t)at[slot[i]]++] = (int32_t)i;
    if ((rc = upload(e, &e->shg_slot_pix, pix.data(), pix.size())) != AOG_OK) return rc;
    if ((rc = upload(e, &e->shg_slot_start, start)) != AOG_OK) return rc;
  }
  if (!separable(e)) {
    if ((rc = need(e, &e->shg_phase, (size_t)e->n_etiles * e->n_ptiles * 1024, true)) != AOG_OK) return rc;
    if (e->sh_pruned && !e->shg_plan) {
      // a pruned handle on the three-pass form keeps neither padded arrays nor a plan: the call's own
      const size_t per = 4 * N2;
      char* p1 = nullptr;
      char* p2 = nullptr;
      if ((rc = dev_alloc(e, &p1, (size_t)B * per * sizeof(float) * 2, true)) != AOG_OK) return rc;
      e->shg_in = p1;
      if ((rc = dev_alloc(e, &p2, (size_t)B * per * sizeof(float) * 2, false)) != AOG_OK) return rc;
      e->shg_pad = p2;
      if ((rc = need(e, &e->shg_tf32, per * 2)) != AOG_OK) return rc;
      hipLaunchKernelGGL(aog::k_shg_tf32, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, nullptr, reinterpret_cast<const double2*>(e->sh_tf),
                         reinterpret_cast<float2*>(e->shg_tf32), per);
      HIP_TRY(hipDeviceSynchronize());
      hipfftHandle plan;
      int dims[2] = {2 * N, 2 * N};
      if (hipfftPlanMany(&plan, 2, dims, nullptr, 1, 4 * N * N, nullptr, 1, 4 * N * N, HIPFFT_C2C, B) != HIPFFT_SUCCESS)
        return fail(AOG_ERR_HIP, "aog_sh_gradient: hipfftPlanMany(C2C %d x %d, batch %d) failed", 2 * N, 2 * N, B);
      e->shg_plan = (void*)(uintptr_t)plan;
    }
  }
  if (values_only) return AOG_OK;
  if ((rc = need(e, &e->shg_gscale, (size_t)2 * B, true)) != AOG_OK) return rc;
  if (separable(e)) {
    if ((rc = need(e, &e->shg_qgrid, (size_t)B * N2, true)) != AOG_OK) return rc;
    if ((rc = need(e, &e->shg_qscale, (size_t)B, true)) != AOG_OK) return rc;
    if ((rc = need(e, &e->shg_slabs, (size_t)aog::pupil_chunks(e->n_ptiles) * e->A_pad * e->Bp, true)) != AOG_OK) return rc;
    if (!e->focal_ap_yx && (rc = upload(e, &e->focal_ap_yx, ap_yx_table(e))) != AOG_OK) return rc;   // (k_grad_obs_backward's gather)
  } else {
    if ((rc = need(e, &e->shg_q64, (size_t)B * e->n_ap, true)) != AOG_OK) return rc;
    if ((rc = need(e, &e->shg_slabs, (size_t)e->A * e->Bp, true)) != AOG_OK) return rc;
  }
  return AOG_OK;
}

// ---- separable route: the forward passes of aog_sh_image as they stand, into the call's image; the phase grid and G1 are the handle's
// (every aog_sh_image call rewrites all it reads of them) ----
template <int RL, int LW>
int forward_sep(aog_env* e, hipStream_t s, double scale) {
  constexpr int BC = 64 / RL;
  const int N = e->cfg.n_pupil;
  const size_t lds = sizeof(float) * 64 * 65 * aog::kShFftWaves, lds_rows = lds + aog::kShHxLdsBytes<RL, LW>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(aog::k_sh_rows_sep<RL, LW>), lds_rows, e->device)) return rc;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(aog::k_sh_cols_sep<RL, LW, false>), lds, e->device)) return rc;
  const dim3 g1((N / BC + aog::kShFftWaves - 1) / aog::kShFftWaves, e->B);
  hipLaunchKernelGGL((aog::k_sh_rows_sep<RL, LW>), g1, dim3(64 * aog::kShFftWaves), lds_rows, s, static_cast<const float*>(e->sh_in),
                     static_cast<float2*>(e->sh_pad), reinterpret_cast<const float2*>(e->sh_tw), reinterpret_cast<const float2*>(e->sh_hxq), (float)e->sh_amp);
  hipLaunchKernelGGL((aog::k_sh_cols_sep<RL, LW, false>), g1, dim3(64 * aog::kShFftWaves), lds, s, static_cast<const float2*>(e->sh_pad), e->shg_image,
                     reinterpret_cast<const float2*>(e->sh_tw), reinterpret_cast<const float2*>(e->sh_hyq), scale, aog::ShFuseArgs{});
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}
template <int RL, int LW>
int backward_sep(aog_env* e, hipStream_t s, const aog::ShGradCot& c, float rs, const uint8_t* mask) {
  constexpr int BC = 64 / RL;
  const int N = e->cfg.n_pupil;
  const size_t lds = sizeof(float) * 64 * 65 * aog::kShFftWaves, lds_rows = lds + aog::kShHxLdsBytes<RL, LW>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(aog::k_shg_cols_back<RL, LW>), lds, e->device)) return rc;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(aog::k_shg_rows_back<RL, LW>), lds_rows, e->device)) return rc;
  const dim3 g1((N / BC + aog::kShFftWaves - 1) / aog::kShFftWaves, e->B);
  hipLaunchKernelGGL((aog::k_shg_cols_back<RL, LW>), g1, dim3(64 * aog::kShFftWaves), lds, s, static_cast<float2*>(e->sh_pad),
                     reinterpret_cast<const float2*>(e->sh_tw), reinterpret_cast<const float2*>(e->sh_hyq), c, e->shg_gscale + e->B, rs, mask);
  hipLaunchKernelGGL((aog::k_shg_rows_back<RL, LW>), g1, dim3(64 * aog::kShFftWaves), lds_rows, s, static_cast<const float*>(e->sh_in),
                     static_cast<const float2*>(e->sh_pad), e->shg_qgrid, reinterpret_cast<const float2*>(e->sh_tw),
                     reinterpret_cast<const float2*>(e->sh_hxq), mask);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}
template <typename F>
int with_sep_instance(const aog_env* e, F&& f) {
  const int N = e->cfg.n_pupil, rl = e->sh_sep_rl;
  if (N % 64 == 0) return rl == 4 ? f(aog::IC<4>{}, aog::IC<64>{}) : rl == 8 ? f(aog::IC<8>{}, aog::IC<64>{}) : f(aog::IC<16>{}, aog::IC<64>{});
  return rl == 8 ? f(aog::IC<8>{}, aog::IC<60>{}) : f(aog::IC<16>{}, aog::IC<60>{});
}

// ---- generic route ----
struct Padded {
  void* in;
  void* pad;
  const void* tf;
  hipfftHandle plan;
};
Padded padded(const aog_env* e) {
  if (e->sh_pruned) return {e->shg_in, e->shg_pad, e->shg_tf32, (hipfftHandle)(uintptr_t)e->shg_plan};
  return {e->sh_in, e->sh_pad, e->sh_double ? (const void*)e->sh_tf : (const void*)e->sh_tf32, (hipfftHandle)(uintptr_t)e->sh_plan};
}
template <typename CT>
int exec(hipfftHandle plan, CT* in, CT* out, int dir) {
  hipfftResult r;
  if constexpr (std::is_same<CT, double2>::value)
    r = hipfftExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex*>(in), reinterpret_cast<hipfftDoubleComplex*>(out), dir);
  else
    r = hipfftExecC2C(plan, reinterpret_cast<hipfftComplex*>(in), reinterpret_cast<hipfftComplex*>(out), dir);
  return r == HIPFFT_SUCCESS ? AOG_OK : fail(AOG_ERR_HIP, "aog_sh_gradient: hipfftExec failed (%d)", (int)r);
}
// aog_sh_image's launches on the padded grid, into the call's image; v stays in the first N x N corner of pad
template <typename CT>
int forward_generic(aog_env* e, hipStream_t s, double scale) {
  const int N = e->cfg.n_pupil;
  const size_t per = (size_t)4 * N * N;
  const Padded w = padded(e);
  CT* in = static_cast<CT*>(w.in);
  CT* pad = static_cast<CT*>(w.pad);
  if (hipfftSetStream(w.plan, s) != HIPFFT_SUCCESS) return fail(AOG_ERR_HIP, "hipfftSetStream failed");
  launch_phase(e, s, e->shg_act16, e->shg_phase);
  const dim3 g_ap((e->n_ap + 255) / 256, e->B), g_per((unsigned)((per + 255) / 256), e->B), g_img((N * N + 255) / 256, e->B);
  hipLaunchKernelGGL(aog::k_sh_field<CT>, g_ap, dim3(256), 0, s, e->shg_phase, e->ap_index, reinterpret_cast<const double2*>(e->sh_mla), in, e->n_ap,
                     e->n_ptiles, N, e->sh_amp, per, 2 * N);
  HIP_TRY(hipGetLastError());
  if (int rc = exec<CT>(w.plan, in, pad, HIPFFT_FORWARD)) return rc;
  hipLaunchKernelGGL(aog::k_sh_transfer<CT>, g_per, dim3(256), 0, s, pad, static_cast<const CT*>(w.tf), per);
  if (int rc = exec<CT>(w.plan, pad, pad, HIPFFT_BACKWARD)) return rc;
  hipLaunchKernelGGL(aog::k_sh_intensity<CT>, g_img, dim3(256), 0, s, pad, e->shg_image, N, scale);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}
template <typename CT>
int backward_generic(aog_env* e, hipStream_t s, const aog::ShGradCot& c, double rs, const uint8_t* mask) {
  const int N = e->cfg.n_pupil;
  const size_t per = (size_t)4 * N * N;
  const Padded w = padded(e);
  CT* pad = static_cast<CT*>(w.pad);
  const dim3 g_ap((e->n_ap + 255) / 256, e->B), g_per((unsigned)((per + 255) / 256), e->B);
  hipLaunchKernelGGL(aog::k_shg_gv<CT>, g_per, dim3(256), 0, s, pad, c, e->shg_gscale + e->B, rs, mask);
  HIP_TRY(hipGetLastError());
  if (int rc = exec<CT>(w.plan, pad, pad, HIPFFT_FORWARD)) return rc;
  hipLaunchKernelGGL(aog::k_shg_transfer_conj<CT>, g_per, dim3(256), 0, s, pad, static_cast<const CT*>(w.tf), per, mask);
  if (int rc = exec<CT>(w.plan, pad, pad, HIPFFT_BACKWARD)) return rc;
  hipLaunchKernelGGL(aog::k_shg_q<CT>, g_ap, dim3(256), 0, s, pad, e->shg_phase, e->ap_index, reinterpret_cast<const double2*>(e->sh_mla), e->shg_q64, e->n_ap,
                     e->n_ptiles, N, mask);
  hipLaunchKernelGGL(aog::k_shg_modes, dim3(e->B), dim3(256), 0, s, e->modes_f32, e->shg_q64, e->shg_slabs, e->n_ap, e->A, e->A_pad, e->Bp, mask);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_sh_gradient(aog_env* e, const uint8_t* mask_dev, const double* g_image_dev, const double* g_slopes_dev, const double* act_dev, double* grad_dev,
                    double* image_dev, double* slopes_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_sh_gradient: null argument");
  const bool values_only = !grad_dev && !g_image_dev && !g_slopes_dev && (image_dev || slopes_dev);
  if (!grad_dev && !values_only) return fail(AOG_ERR_INVALID, "aog_sh_gradient: grad_dev is null (allowed only with no cotangent, for the values alone)");
  if (!values_only && !g_image_dev && !g_slopes_dev) return fail(AOG_ERR_INVALID, "aog_sh_gradient: both cotangent pointers are null");
  if (int rc = instrument_gate(e, "aog_sh_gradient", e->sh_ready, "the Shack-Hartmann chain was", "aog_upload_sh")) return rc;
  const bool sep = separable(e);
  if (sep && !values_only && (!e->grad_ready || !e->grad_mtab16))
    return fail(AOG_ERR_STATE, "aog_sh_gradient: handles on the separable propagation contract with the modes operands of aog_upload_gradient (call it "
                "first, again after aog_upload_tables)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = e->cfg.n_pupil, B = e->B, n_sub = e->sh_n_sub;
  const size_t N2 = (size_t)N * N;
  int rc;
  if ((rc = grad_buffers(e, values_only)) != AOG_OK) return rc;
  if ((rc = ensure_tiles(e, s)) != AOG_OK) return rc;
  // the point of evaluation in the operand layout, then the forward chain into the call's own image
  {
    const int n = B * e->A_pad;
    hipLaunchKernelGGL(aog::k_shg_act16, dim3((n + 255) / 256), dim3(256), 0, s, act_dev ? act_dev : e->sh_act, e->shg_act16, B, e->A, e->A_pad,
                       2.0 / e->cfg.wavelength_wfs);
  }
  const double norm = 1.0 / (double)(4 * N2), scale = e->sh_scale * norm * norm;
  if (sep) {
    launch_phase_field(e, s, e->shg_act16, static_cast<float*>(e->sh_in), N2, N, true);
    rc = with_sep_instance(e, [&](auto rlc, auto lwc) { return forward_sep<decltype(rlc)::v, decltype(lwc)::v>(e, s, scale); });
  } else {
    rc = e->sh_double ? forward_generic<double2>(e, s, scale) : forward_generic<float2>(e, s, scale);
  }
  if (rc) return rc;
  aog::ShGradCentroidArgs ca{};
  ca.image = e->shg_image;
  ca.slot_start = e->shg_slot_start;
  ca.slot_pix = e->shg_slot_pix;
  ca.x_det = e->sh_xdet;
  ca.centres = e->sh_centres;
  ca.slopes_ref = e->sh_ref;
  ca.g_slopes = g_slopes_dev;
  ca.coef = e->shg_coef;
  ca.slopes_out = slopes_dev;
  ca.mask = mask_dev;
  ca.N = N;
  ca.n_sub = n_sub;
  hipLaunchKernelGGL(aog::k_shg_centroids, dim3(n_sub, B), dim3(64), 0, s, ca);
  if (image_dev) hipLaunchKernelGGL(aog::k_shg_copy_rows, dim3((unsigned)((N2 + 255) / 256), B), dim3(256), 0, s, e->shg_image, image_dev, N2, mask_dev);
  HIP_TRY(hipGetLastError());
  if (values_only) return AOG_OK;
  aog::ShGradCot c{};
  c.g_image = g_image_dev;
  c.coef = e->shg_coef;
  c.sub_slot = e->sh_slot;
  c.x_det = e->sh_xdet;
  c.N = N;
  c.n_sub = n_sub;
  hipLaunchKernelGGL(aog::k_shg_cotscale, dim3(B), dim3(256), 0, s, c, e->shg_gscale, B, mask_dev);
  // dL/da = (4 pi / lambda) sum_p M_pk g_phi_p with g_phi = 2 amplitude sqrt(scale) gscale q (k_shack_back.h)
  const double rs64 = std::sqrt(scale);
  const float rs32 = (float)rs64;
  aog::ShGradFinishArgs f{};
  f.slabs = e->shg_slabs;
  f.grad = grad_dev;
  f.mask = mask_dev;
  f.Bp = e->Bp;
  f.A = e->A;
  f.gscale = e->shg_gscale;
  f.factor = 4.0 * M_PI / e->cfg.wavelength_wfs * 2.0 * e->sh_amp;
  if (sep) {
    if ((rc = with_sep_instance(e, [&](auto rlc, auto lwc) { return backward_sep<decltype(rlc)::v, decltype(lwc)::v>(e, s, c, rs32, mask_dev); })) != AOG_OK)
      return rc;
    hipLaunchKernelGGL(aog::k_shg_qnorm, dim3(B), dim3(256), 0, s, e->shg_qgrid, e->focal_ap_yx, e->shg_qscale, N, e->n_ap, mask_dev);
    launch_grad_obs_backward(e, s, e->shg_qgrid, N2, N, 0, B, e->shg_slabs);
    f.qscale = e->shg_qscale;
    f.n_chunks = aog::pupil_chunks(e->n_ptiles);
    f.rows = e->A_pad;
    f.factor *= (double)rs32 / (double)aog::kModeScale;
  } else {
    const double rs = e->sh_double ? rs64 : (double)rs32;
    if ((rc = e->sh_double ? backward_generic<double2>(e, s, c, rs, mask_dev) : backward_generic<float2>(e, s, c, rs, mask_dev)) != AOG_OK) return rc;
    f.qscale = nullptr;
    f.n_chunks = 1;
    f.rows = e->A;
    f.factor *= rs;
  }
  hipLaunchKernelGGL(aog::k_shg_finish, dim3(B), dim3(256), 0, s, f);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
