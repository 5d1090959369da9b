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
  LAUNCH_PLAIN(g->state.device, stream, aog::k_spgd_update, dim3((B + aog::kSpgdEnvs - 1) / aog::kSpgdEnvs), dim3(64 * aog::kSpgdEnvs), s);
  return AOG_OK;
}

int spgd_check(const aog_spgd_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_spgd_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->reserved0 != 0) return fail(AOG_ERR_INVALID, "aog_spgd_create: reserved fields must be 0");
  if (cfg->num_envs < 1 || cfg->act_dim < 1) return fail(AOG_ERR_INVALID, "aog_spgd_create: bad dimensions (num_envs %d, act_dim %d)", cfg->num_envs, cfg->act_dim);
  if (cfg->metric != AOG_SPGD_POWER && cfg->metric != AOG_SPGD_STREHL && cfg->metric != AOG_SPGD_REWARD)
    return fail(AOG_ERR_INVALID, "aog_spgd_create: metric %d (0 = power, 1 = strehl, 2 = reward)", cfg->metric);
  if (!std::isfinite(cfg->clip) || cfg->clip < 0.0) return fail(AOG_ERR_INVALID, "aog_spgd_create: clip %g must be finite and >= 0", cfg->clip);
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_spgd_create(const aog_spgd_config* cfg, int device, aog_spgd** out) {
  // u = 0, J_plus = 0, k = 0, h = 0; gain = amplitude = 0 until aog_spgd_set_params
  return handle_create("aog_spgd_create", cfg, device, out, spgd_check, [](aog_spgd* g) {
    const size_t B = (size_t)g->cfg.num_envs;
    if (hipError_t err = g->alloc_state(aog::spgd_record_doubles(g->cfg.act_dim) * sizeof(double) * B, true)) return err;
    if (hipError_t err = g->own(&g->gain, B * sizeof(double), true)) return err;
    if (hipError_t err = g->own(&g->amplitude, B * sizeof(double), true)) return err;
    return g->own(&g->metric, B * sizeof(float), true);
  });
}

void aog_spgd_destroy(aog_spgd* g) { handle_destroy(g); }

int aog_spgd_set_params(aog_spgd* g, const double* gain_host, const double* amplitude_host) {
  REFUSE_NULL("aog_spgd_set_params", {"spgd", g}, {"gain_host", gain_host}, {"amplitude_host", amplitude_host});
  for (int b = 0; b < g->cfg.num_envs; ++b)
    if (!std::isfinite(gain_host[b]) || gain_host[b] < 0.0 || !std::isfinite(amplitude_host[b]) || amplitude_host[b] < 0.0)
      return fail(AOG_ERR_INVALID, "aog_spgd_set_params: gain and amplitude must be finite and >= 0 (env %d: gain %g, amplitude %g)", b, gain_host[b],
                  amplitude_host[b]);
  HIP_TRY(hipSetDevice(g->state.device));
  HIP_TRY(hipMemcpy(g->gain, gain_host, (size_t)g->cfg.num_envs * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(g->amplitude, amplitude_host, (size_t)g->cfg.num_envs * sizeof(double), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_spgd_reset(aog_spgd* g, const uint8_t* mask_dev, const double* act_dev, float* action_out, void* stream) {
  REFUSE_NULL("aog_spgd_reset", {"spgd", g});
  return launch_query(g, spgd_args(g, true, nullptr, mask_dev, act_dev, action_out), stream);
}

int aog_spgd_update(aog_spgd* g, const float* metric_dev, const uint8_t* mask_dev, float* action_out, void* stream) {
  REFUSE_NULL("aog_spgd_update", {"spgd", g}, {"metric_dev", metric_dev}, {"action_out", action_out});
  return launch_query(g, spgd_args(g, false, metric_dev, mask_dev, nullptr, action_out), stream);
}

int64_t aog_spgd_state_bytes(const aog_spgd* g) { return handle_state_bytes(g); }

int aog_spgd_get_state(aog_spgd* g, void* blob_dev, void* stream) { return handle_get_state("aog_spgd_get_state", "spgd", g, blob_dev, stream); }

int aog_spgd_set_state(aog_spgd* g, const void* blob_dev, void* stream) { return handle_set_state("aog_spgd_set_state", "spgd", g, blob_dev, stream); }

}  // extern "C"
