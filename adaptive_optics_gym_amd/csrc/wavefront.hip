// K12: residual wavefront statistics and the best-fit mirror command (aog_upload_wavefront_fit, aog_wavefront_truth).  A translation unit of
// its own: the kernels a step launches keep their code objects as they are.
#include "host_common.h"
#include "k_wavefront.h"

using namespace aog_host;

extern "C" {

int aog_upload_wavefront_fit(aog_env* e, const double* modes_host, const double* fit_host) {
  if (!e || !modes_host || !fit_host) return fail(AOG_ERR_INVALID, "aog_upload_wavefront_fit: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_wavefront_fit before aog_upload_tables");
  HIP_TRY(hipSetDevice(e->device));
  const int n_ap = e->n_ap, A = e->A;
  e->wf_ready = false;
  int rc;
  std::vector<double> colsum((size_t)A, 0.0);
  for (int p = 0; p < n_ap; ++p)
    for (int k = 0; k < A; ++k) colsum[k] += modes_host[(size_t)p * A + k];
  if ((rc = upload(e, &e->wf_colsum, colsum, true)) != AOG_OK) return rc;
  if ((rc = upload(e, &e->wf_fit, fit_host, (size_t)A * A, true)) != AOG_OK) return rc;
  if (e->cfg.precision == AOG_PRECISION_FAST) {
    // the modes as table operands of the second contraction, scaled like modes16
    const std::vector<_Float16> t16 = pack_tab16_rows(e->n_ptiles, n_ap, A, aog::pupil_blocks(e->A_pad), aog::kModeScale,
                                                      [&](int p, int k) { return modes_host[(size_t)p * A + k]; });
    if ((rc = upload(e, &e->wf_tab16, t16, true)) != AOG_OK) return rc;
  }
  e->wf_ready = true;
  return AOG_OK;
}

int aog_wavefront_truth(aog_env* e, double* rms_dev, double* fit_rms_dev, double* coef_dev, double* act_ideal_dev, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_wavefront_truth: null argument");
  if (!rms_dev && !fit_rms_dev && !coef_dev && !act_ideal_dev) return fail(AOG_ERR_INVALID, "aog_wavefront_truth: every output pointer is null");
  if (int rc = instrument_gate(e, "aog_wavefront_truth", e->wf_ready, "the wavefront fit was", "aog_upload_wavefront_fit")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
  const int n_chunks = fast ? aog::pupil_chunks(e->n_ptiles) : 1, rows = e->A_pad + 2;
  int rc;
  // work buffers of the call's own, on first use (never initialised: every element that is read is written by the call first)
  if (!e->wf_slabs && (rc = dev_alloc(e, &e->wf_slabs, (size_t)n_chunks * rows * e->Bp, false)) != AOG_OK) return rc;
  if (fast) {
    if ((rc = instrument_operands(e, s, false)) != AOG_OK) return rc;
    with_apad(e->A_pad, [&](auto apad) {
      hipLaunchKernelGGL((aog::k_wavefront_fit<apad()>), dim3(n_chunks, e->n_etiles), dim3(256), 0, s, reinterpret_cast<const aog::f16x8*>(e->modes16),
                         reinterpret_cast<const aog::f16x8*>(e->wf_tab16), reinterpret_cast<const aog::f32x4*>(e->psi_tile),
                         reinterpret_cast<const aog::f16x8*>(e->inst_act16), e->wf_slabs, e->n_ptiles, e->n_ap, e->Bp);
    });
  } else {
    if (!e->wf_w && (rc = dev_alloc(e, &e->wf_w, (size_t)e->B * e->n_ap, false)) != AOG_OK) return rc;
    hipLaunchKernelGGL(aog::k_wavefront_ref, dim3(e->B), dim3(256), 0, s, e->modes64, e->psi64, e->act_dm, e->wf_w, e->wf_slabs, e->n_ap, e->A, rows,
                       e->Bp);
  }
  HIP_TRY(hipGetLastError());
  aog::WavefrontFinishArgs p{};
  p.slabs = e->wf_slabs;
  p.fit = e->wf_fit;
  p.colsum = e->wf_colsum;
  p.act_dm = e->act_dm;
  p.rms = rms_dev;
  p.fit_rms = fit_rms_dev;
  p.coef = coef_dev;
  p.act_ideal = act_ideal_dev;
  p.n_chunks = n_chunks;
  p.rows = rows;
  p.Bp = e->Bp;
  p.A = e->A;
  p.n_ap = e->n_ap;
  p.scale = fast ? e->cfg.wavelength_wfs : 1.0;
  hipLaunchKernelGGL(aog::k_wavefront_finish, dim3(e->B), dim3(256), 0, s, p);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
