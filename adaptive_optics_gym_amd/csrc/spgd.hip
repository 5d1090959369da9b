// K19: the SPGD controller's own entry points (aog_spgd_*): handle, parameters, stand-alone query and reset, checkpointing.  The fused
// step tail (aog_reset_spgd / aog_step_spgd) is launched from aogym.hip.
#include "spgd_host.h"

using namespace aog_host;

namespace aog {
// The stand-alone query (aog_spgd_update, aog_spgd_reset): one wave per env, kSpgdEnvs per workgroup.
__global__ __launch_bounds__(64 * kSpgdEnvs) void k_spgd_update(SpgdArgs s) {
  const int env = (int)blockIdx.x * kSpgdEnvs + (int)(threadIdx.x >> 6);
  if (env >= s.B || (s.mask && !s.mask[env])) return;   // (uniform per wave)
  spgd_query(s, env, (int)(threadIdx.x & 63));
}
}  // namespace aog

namespace {

int launch_query(const aog_spgd* g, const aog::SpgdArgs& s, void* stream) {
  const int B = g->cfg.num_envs;
  LAUNCH_PLAIN(g->device, stream, aog::k_spgd_update, dim3((B + aog::kSpgdEnvs - 1) / aog::kSpgdEnvs), dim3(64 * aog::kSpgdEnvs), s);
  return AOG_OK;
}

void release(aog_spgd* g) {
  g->state.release();
  if (g->gain) (void)hipFree(g->gain);
  if (g->amplitude) (void)hipFree(g->amplitude);
  if (g->metric) (void)hipFree(g->metric);
  delete g;
}

}  // namespace

extern "C" {

int aog_spgd_create(const aog_spgd_config* cfg, int device, aog_spgd** out) {
  if (!cfg || !out) return fail(AOG_ERR_INVALID, "aog_spgd_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_spgd_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->reserved0 != 0) return fail(AOG_ERR_INVALID, "aog_spgd_create: reserved fields must be 0");
  if (cfg->num_envs < 1 || cfg->act_dim < 1) return fail(AOG_ERR_INVALID, "aog_spgd_create: bad dimensions (num_envs %d, act_dim %d)", cfg->num_envs, cfg->act_dim);
  if (cfg->metric != AOG_SPGD_POWER && cfg->metric != AOG_SPGD_STREHL && cfg->metric != AOG_SPGD_REWARD)
    return fail(AOG_ERR_INVALID, "aog_spgd_create: metric %d (0 = power, 1 = strehl, 2 = reward)", cfg->metric);
  if (!std::isfinite(cfg->clip) || cfg->clip < 0.0) return fail(AOG_ERR_INVALID, "aog_spgd_create: clip %g must be finite and >= 0", cfg->clip);
  HIP_TRY(hipSetDevice(device));
  aog_spgd* g = new aog_spgd;
  g->cfg = *cfg;
  g->device = device;
  const size_t B = (size_t)cfg->num_envs;
  hipError_t err = g->state.alloc(device, aog::spgd_record_doubles(cfg->act_dim) * sizeof(double) * B);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&g->gain), B * sizeof(double));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&g->amplitude), B * sizeof(double));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&g->metric), B * sizeof(float));
  // u = 0, J_plus = 0, k = 0, h = 0; gain = amplitude = 0 until aog_spgd_set_params
  if (err == hipSuccess) err = hipMemset(g->state.ptr, 0, g->state.bytes);
  if (err == hipSuccess) err = hipMemset(g->gain, 0, B * sizeof(double));
  if (err == hipSuccess) err = hipMemset(g->amplitude, 0, B * sizeof(double));
  if (err == hipSuccess) err = hipMemset(g->metric, 0, B * sizeof(float));
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    release(g);
    return fail(AOG_ERR_HIP, "aog_spgd_create: %s", hipGetErrorString(err));
  }
  *out = g;
  return AOG_OK;
}

void aog_spgd_destroy(aog_spgd* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  release(g);
}

int aog_spgd_set_params(aog_spgd* g, const double* gain_host, const double* amplitude_host) {
  if (!g || !gain_host || !amplitude_host) return fail(AOG_ERR_INVALID, "aog_spgd_set_params: null argument");
  for (int b = 0; b < g->cfg.num_envs; ++b)
    if (!std::isfinite(gain_host[b]) || gain_host[b] < 0.0 || !std::isfinite(amplitude_host[b]) || amplitude_host[b] < 0.0)
      return fail(AOG_ERR_INVALID, "aog_spgd_set_params: gain and amplitude must be finite and >= 0 (env %d: gain %g, amplitude %g)", b, gain_host[b],
                  amplitude_host[b]);
  HIP_TRY(hipSetDevice(g->device));
  HIP_TRY(hipMemcpy(g->gain, gain_host, (size_t)g->cfg.num_envs * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(g->amplitude, amplitude_host, (size_t)g->cfg.num_envs * sizeof(double), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_spgd_reset(aog_spgd* g, const uint8_t* mask_dev, const double* act_dev, float* action_out, void* stream) {
  if (!g) return fail(AOG_ERR_INVALID, "aog_spgd_reset: null argument");
  return launch_query(g, spgd_args(g, true, nullptr, mask_dev, act_dev, action_out), stream);
}

int aog_spgd_update(aog_spgd* g, const float* metric_dev, const uint8_t* mask_dev, float* action_out, void* stream) {
  if (!g || !metric_dev || !action_out) return fail(AOG_ERR_INVALID, "aog_spgd_update: null argument");
  return launch_query(g, spgd_args(g, false, metric_dev, mask_dev, nullptr, action_out), stream);
}

int64_t aog_spgd_state_bytes(const aog_spgd* g) { return g ? (int64_t)g->state.bytes : 0; }

int aog_spgd_get_state(aog_spgd* g, void* blob_dev, void* stream) {
  if (!g || !blob_dev) return fail(AOG_ERR_INVALID, "aog_spgd_get_state: null argument");
  return g->state.copy_out(blob_dev, stream);
}

int aog_spgd_set_state(aog_spgd* g, const void* blob_dev, void* stream) {
  if (!g || !blob_dev) return fail(AOG_ERR_INVALID, "aog_spgd_set_state: null argument");
  return g->state.copy_in(blob_dev, stream);
}

}  // extern "C"
