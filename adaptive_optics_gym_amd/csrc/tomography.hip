// K24: tomography (include/aogym_tomography.h).  aog_upload_wavefront_shapes / aog_wavefront_project: a front's residual wavefront projected
// onto a caller's shapes, an off-step instrument of aog_env beside K12.  aog_tomo_*: the reconstructor and integrator, a handle of its own.
// A translation unit of its own: the kernels a step launches keep their code objects as they are.
#include "standalone_handle.h"
#include "k_tomography.h"
#include "../../include/aogym_tomography.h"

using namespace aog_host;

struct aog_tomo : StandaloneHandle<aog_tomo_config> {   // state: u [B][K] float64
  double* R[AOG_TOMO_MAX_INPUTS] = {nullptr, nullptr, nullptr, nullptr};   // [K][J_g]
};

namespace {

// f(std::integral_constant<int, 1 .. 4>) for the blocks of a row group
template <typename F>
void with_gblk(int gblk, F&& f) {
  switch (gblk) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

size_t envs(const aog_tomo* t) { return (size_t)t->cfg.num_envs; }
size_t outs(const aog_tomo* t) { return (size_t)t->cfg.n_out; }
double* command(const aog_tomo* t) { return reinterpret_cast<double*>(t->state.ptr); }

int tomo_check(const aog_tomo_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION)
    return fail(AOG_ERR_INVALID, "aog_tomo_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_tomo_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->n_out < 1 || cfg->n_out > AOG_TOMO_MAX_OUT) return fail(AOG_ERR_INVALID, "aog_tomo_create: n_out %d outside [1, %d]", cfg->n_out, AOG_TOMO_MAX_OUT);
  if (cfg->n_inputs < 1 || cfg->n_inputs > AOG_TOMO_MAX_INPUTS)
    return fail(AOG_ERR_INVALID, "aog_tomo_create: n_inputs %d outside [1, %d]", cfg->n_inputs, AOG_TOMO_MAX_INPUTS);
  for (int g = 0; g < AOG_TOMO_MAX_INPUTS; ++g) {
    if (g < cfg->n_inputs && (cfg->width[g] < 1 || cfg->width[g] > AOG_TOMO_MAX_WIDTH))
      return fail(AOG_ERR_INVALID, "aog_tomo_create: width[%d] %d outside [1, %d]", g, cfg->width[g], AOG_TOMO_MAX_WIDTH);
    if (g >= cfg->n_inputs && cfg->width[g] != 0) return fail(AOG_ERR_INVALID, "aog_tomo_create: width[%d] must be 0 beyond n_inputs %d", g, cfg->n_inputs);
  }
  if (cfg->env_id_base < 0) return fail(AOG_ERR_INVALID, "aog_tomo_create: env_id_base %d must be >= 0", cfg->env_id_base);
  if (cfg->reserved != 0) return fail(AOG_ERR_INVALID, "aog_tomo_create: reserved must be 0");
  // (the kernels number commands and inputs with 32-bit integers)
  if ((long long)cfg->num_envs * AOG_TOMO_MAX_OUT > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "aog_tomo_create: num_envs %d x %d exceeds 2^31 - 1 values", cfg->num_envs, AOG_TOMO_MAX_OUT);
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_upload_wavefront_shapes(aog_env* e, const double* shapes_host, int K) {
  if (!e || !shapes_host) return fail(AOG_ERR_INVALID, "aog_upload_wavefront_shapes: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_upload_wavefront_shapes before aog_upload_tables");
  if (K < 1 || K > AOG_WAVEFRONT_MAX_SHAPES) return fail(AOG_ERR_INVALID, "aog_upload_wavefront_shapes: n_shapes %d outside [1, %d]", K, AOG_WAVEFRONT_MAX_SHAPES);
  const int n_ap = e->n_ap;
  double largest = 0.0;
  std::vector<double> rowsum((size_t)K, 0.0);
  for (int k = 0; k < K; ++k)
    for (int p = 0; p < n_ap; ++p) {
      const double v = shapes_host[(size_t)k * n_ap + p];
      if (!std::isfinite(v)) return fail(AOG_ERR_INVALID, "aog_upload_wavefront_shapes: shapes[%d][%d] is not finite", k, p);
      largest = std::max(largest, std::fabs(v));
      rowsum[k] += v;
    }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // (a projection in flight reads the buffers released below)
  e->tomo_ready = false;
  dev_release(e, &e->tomo_tab16);
  dev_release(e, &e->tomo_shapes64);
  dev_release(e, &e->tomo_rowsum);
  dev_release(e, &e->tomo_slabs);
  int rc;
  if ((rc = upload(e, &e->tomo_rowsum, rowsum)) != AOG_OK) return rc;
  if (e->cfg.precision == AOG_PRECISION_FAST) {
    // the operand scale of this upload: the power of two that brings the largest |S| into [2^13, 2^14), kModeScale's place for unit modes
    int exp2 = 0;
    if (largest > 0.0) (void)std::frexp(largest, &exp2);
    const int shift = std::min(120, std::max(-120, 14 - exp2));
    const double scale = std::ldexp(1.0, shift);
    const int nblk = (K + 31) / 32;
    e->tomo_groups = (nblk + aog::kProjectMaxBlocks - 1) / aog::kProjectMaxBlocks;
    e->tomo_gblk = (nblk + e->tomo_groups - 1) / e->tomo_groups;
    e->tomo_unscale = 1.0 / (scale * (double)aog::kActScale);
    const int grows = 32 * e->tomo_gblk;
    std::vector<_Float16> t16;
    for (int g = 0; g < e->tomo_groups; ++g) {
      const int k0 = g * grows, rows = std::min(grows, K - k0);
      const std::vector<_Float16> part = pack_tab16_rows(e->n_ptiles, n_ap, rows, e->tomo_gblk, 1.0f,
                                                         [&](int p, int k) { return shapes_host[(size_t)(k0 + k) * n_ap + p] * scale; });
      t16.insert(t16.end(), part.begin(), part.end());
    }
    if ((rc = upload(e, &e->tomo_tab16, t16)) != AOG_OK) return rc;
    const size_t slab = (size_t)e->tomo_groups * aog::pupil_chunks(e->n_ptiles) * (grows + 1) * e->Bp;
    if ((rc = dev_alloc(e, &e->tomo_slabs, slab, false)) != AOG_OK) return rc;
  } else {
    std::vector<double> t((size_t)n_ap * K);
    for (int k = 0; k < K; ++k)
      for (int p = 0; p < n_ap; ++p) t[(size_t)p * K + k] = shapes_host[(size_t)k * n_ap + p];
    if ((rc = upload(e, &e->tomo_shapes64, t)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->tomo_slabs, (size_t)(K + 1) * e->Bp, false)) != AOG_OK) return rc;
  }
  e->tomo_K = K;
  e->tomo_ready = true;
  return AOG_OK;
}

int aog_wavefront_project(aog_env* e, double* out_dev, double* mean_dev, void* stream) {
  if (!e || !out_dev) return fail(AOG_ERR_INVALID, "aog_wavefront_project: null argument");
  if (int rc = instrument_gate(e, "aog_wavefront_project", e->tomo_ready, "the shapes were", "aog_upload_wavefront_shapes")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
  const int K = e->tomo_K;
  int rc;
  aog::ProjectFinishArgs p{};
  if (fast) {
    if ((rc = instrument_operands(e, s, false)) != AOG_OK) return rc;
    const int n_chunks = aog::pupil_chunks(e->n_ptiles);
    with_apad(e->A_pad, [&](auto apad) {
      with_gblk(e->tomo_gblk, [&](auto gblk) {
        hipLaunchKernelGGL((aog::k_wavefront_project<apad(), gblk()>), dim3(n_chunks, e->n_etiles, e->tomo_groups), dim3(256), 0, s,
                           reinterpret_cast<const aog::f16x8*>(e->modes16), reinterpret_cast<const aog::f16x8*>(e->tomo_tab16),
                           reinterpret_cast<const aog::f32x4*>(e->psi_tile), reinterpret_cast<const aog::f16x8*>(e->inst_act16), e->tomo_slabs,
                           e->n_ptiles, e->n_ap, e->Bp, e->tomo_unscale);
      });
    });
    p.n_chunks = n_chunks;
    p.rows = 32 * e->tomo_gblk + 1;
    p.scale = e->cfg.wavelength_wfs;
  } else {
    if ((rc = need(e, &e->wf_w, (size_t)e->B * e->n_ap)) != AOG_OK) return rc;
    hipLaunchKernelGGL(aog::k_project_ref, dim3(e->B), dim3(256), 0, s, e->modes64, e->tomo_shapes64, e->psi64, e->act_dm, e->wf_w, e->tomo_slabs,
                       e->n_ap, e->A, K, e->Bp);
    p.n_chunks = 1;
    p.rows = K + 1;
    p.scale = 1.0;
  }
  HIP_TRY(hipGetLastError());
  p.slabs = e->tomo_slabs;
  p.rowsum = e->tomo_rowsum;
  p.out = out_dev;
  p.mean = mean_dev;
  p.Bp = e->Bp;
  p.K = K;
  p.n_ap = e->n_ap;
  hipLaunchKernelGGL(aog::k_project_finish, dim3(e->B), dim3(256), 0, s, p);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int64_t aog_tomo_config_size(void) { return (int64_t)sizeof(aog_tomo_config); }

int aog_tomo_create(const aog_tomo_config* cfg, int device, aog_tomo** out) {
  // the command and the matrices start as zeros
  return handle_create("aog_tomo_create", cfg, device, out, tomo_check, [](aog_tomo* t) {
    if (hipError_t err = t->alloc_state(sizeof(double) * envs(t) * outs(t), true)) return err;
    for (int g = 0; g < t->cfg.n_inputs; ++g)
      if (hipError_t err = t->own(&t->R[g], sizeof(double) * outs(t) * t->cfg.width[g], true)) return err;
    return hipSuccess;
  });
}

void aog_tomo_destroy(aog_tomo* t) { handle_destroy(t); }

int aog_tomo_upload(aog_tomo* t, int g, const double* R_dev, void* stream) {
  REFUSE_NULL("aog_tomo_upload", {"tomo", t}, {"R_dev", R_dev});
  if (g < 0 || g >= t->cfg.n_inputs) return fail(AOG_ERR_INVALID, "aog_tomo_upload: g %d outside [0, n_inputs = %d)", g, t->cfg.n_inputs);
  HIP_TRY(hipSetDevice(t->state.device));
  HIP_TRY(hipMemcpyAsync(t->R[g], R_dev, sizeof(double) * outs(t) * t->cfg.width[g], hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return AOG_OK;
}

int aog_tomo_update(aog_tomo* t, const double* const* inputs_host, double gain, double leak, double stroke, const uint8_t* mask_dev,
                    double* out_u_dev, void* stream) {
  REFUSE_NULL("aog_tomo_update", {"tomo", t}, {"inputs_host", inputs_host});
  if (!std::isfinite(gain)) return fail(AOG_ERR_INVALID, "aog_tomo_update: gain %g is not finite", gain);
  if (!std::isfinite(leak)) return fail(AOG_ERR_INVALID, "aog_tomo_update: leak %g is not finite", leak);
  if (std::isnan(stroke)) return fail(AOG_ERR_INVALID, "aog_tomo_update: stroke is NaN (<= 0: no clip)");
  aog::TomoArgs a{};
  for (int g = 0; g < t->cfg.n_inputs; ++g) {
    if (!inputs_host[g]) return fail(AOG_ERR_INVALID, "aog_tomo_update: null argument inputs_host[%d]", g);
    a.R[g] = t->R[g];
    a.s[g] = inputs_host[g];
    a.J[g] = t->cfg.width[g];
  }
  a.u = command(t);
  a.out = out_u_dev;
  a.mask = mask_dev;
  a.B = t->cfg.num_envs;
  a.K = t->cfg.n_out;
  a.G = t->cfg.n_inputs;
  a.gain = gain;
  a.leak = leak;
  a.stroke = stroke;
  const dim3 grid((unsigned)((a.B + aog::kTomoEnvs - 1) / aog::kTomoEnvs), (unsigned)((a.K + aog::kTomoOuts - 1) / aog::kTomoOuts));
  LAUNCH_PLAIN(t->state.device, stream, aog::k_tomo_update, grid, dim3(256), a);
  return AOG_OK;
}

int aog_tomo_reset(aog_tomo* t, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_tomo_reset", {"tomo", t});
  const int n = t->cfg.num_envs * t->cfg.n_out;
  LAUNCH_PLAIN(t->state.device, stream, aog::k_tomo_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), command(t), mask_dev, t->cfg.num_envs, t->cfg.n_out);
  return AOG_OK;
}

int64_t aog_tomo_state_bytes(const aog_tomo* t) { return handle_state_bytes(t); }

int aog_tomo_get_state(aog_tomo* t, void* blob_dev, void* stream) { return handle_get_state("aog_tomo_get_state", "tomo", t, blob_dev, stream); }

int aog_tomo_set_state(aog_tomo* t, const void* blob_dev, void* stream) { return handle_set_state("aog_tomo_set_state", "tomo", t, blob_dev, stream); }

}  // extern "C"
