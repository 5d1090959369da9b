// K25: the LQG controller (include/aogym_lqg.h): per (env, mode) a steady-state Kalman filter on turbulence plus vibration lines that
// predicts `delay` frames ahead.  Independent of any aog_env; whoever owns the handle feeds it pseudo-open-loop measurements.
#include "standalone_handle.h"
#include "k_lqg.h"
#include "../../include/aogym_lqg.h"

using namespace aog_host;

struct aog_lqg : StandaloneHandle<aog_lqg_config> {   // state: the records [B][9 S + 4][A] float64 (k_lqg.h)
  int* all_solved = nullptr;   // what k_lqg_all_solved writes for aog_lqg_set_state
  bool solved = false;         // aog_lqg_solve has run since the last aog_lqg_set_model
};

namespace {

// f(std::integral_constant<int, 1 .. 4>) for the number of sub-models
template <typename F>
void with_models(int S, F&& f) {
  switch (S) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

double* records(const aog_lqg* g) { return reinterpret_cast<double*>(g->state.ptr); }
dim3 grid_of(const aog_lqg* g) { return dim3((unsigned)(((size_t)g->cfg.num_envs * g->cfg.act_dim + 255) / 256)); }

int lqg_check(const aog_lqg_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_lqg_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_lqg_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->act_dim < 1 || cfg->act_dim > AOG_LQG_MAX_ACT) return fail(AOG_ERR_INVALID, "aog_lqg_create: act_dim %d outside [1, %d]", cfg->act_dim, AOG_LQG_MAX_ACT);
  if (cfg->n_models < 1 || cfg->n_models > AOG_LQG_MAX_MODELS)
    return fail(AOG_ERR_INVALID, "aog_lqg_create: n_models %d outside [1, %d]", cfg->n_models, AOG_LQG_MAX_MODELS);
  if (cfg->reserved != 0) return fail(AOG_ERR_INVALID, "aog_lqg_create: reserved must be 0");
  // (the kernels number the (env, mode) cells of a launch with 32-bit env and mode numbers)
  if ((long long)cfg->num_envs * AOG_LQG_MAX_ACT > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "aog_lqg_create: num_envs %d x %d exceeds 2^31 - 1 cells", cfg->num_envs, AOG_LQG_MAX_ACT);
  return AOG_OK;
}

}  // namespace

extern "C" {

int64_t aog_lqg_config_size(void) { return (int64_t)sizeof(aog_lqg_config); }

int aog_lqg_create(const aog_lqg_config* cfg, int device, aog_lqg** out) {
  // the records start as zeros: no model, no gains
  return handle_create("aog_lqg_create", cfg, device, out, lqg_check, [](aog_lqg* g) {
    const size_t cells = (size_t)g->cfg.num_envs * g->cfg.act_dim;
    if (hipError_t err = g->alloc_state(sizeof(double) * cells * aog::lqg_rows(g->cfg.n_models), true)) return err;
    return g->own(&g->all_solved, sizeof(int), true);
  });
}

void aog_lqg_destroy(aog_lqg* g) { handle_destroy(g); }

int aog_lqg_set_model(aog_lqg* g, const double* a_dev, const double* q_dev, const double* r_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_lqg_set_model", {"lqg", g}, {"a_dev", a_dev}, {"q_dev", q_dev}, {"r_dev", r_dev});
  g->solved = false;
  LAUNCH_PLAIN(g->state.device, stream, aog::k_lqg_set_model, grid_of(g), dim3(256), records(g), a_dev, q_dev, r_dev, mask_dev, g->cfg.num_envs,
               g->cfg.act_dim, g->cfg.n_models);
  return AOG_OK;
}

int aog_lqg_solve(aog_lqg* g, int delay, int iterations, double* convergence_out_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_lqg_solve", {"lqg", g});
  if (delay < 1 || delay > AOG_LQG_MAX_DELAY) return fail(AOG_ERR_INVALID, "aog_lqg_solve: delay %d outside [1, %d]", delay, AOG_LQG_MAX_DELAY);
  if (iterations < 1 || iterations > AOG_LQG_MAX_ITERATIONS)
    return fail(AOG_ERR_INVALID, "aog_lqg_solve: iterations %d outside [1, %d]", iterations, AOG_LQG_MAX_ITERATIONS);
  HIP_TRY(hipSetDevice(g->state.device));
  with_models(g->cfg.n_models, [&](auto S) {
    hipLaunchKernelGGL(aog::k_lqg_solve<S()>, grid_of(g), dim3(256), 0, static_cast<hipStream_t>(stream), records(g), convergence_out_dev, mask_dev,
                       g->cfg.num_envs, g->cfg.act_dim, delay, iterations);
  });
  HIP_TRY(hipGetLastError());
  g->solved = true;
  return AOG_OK;
}

int aog_lqg_update(aog_lqg* g, const double* y_dev, double* out_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_lqg_update", {"lqg", g}, {"y_dev", y_dev}, {"out_dev", out_dev});
  if (!g->solved) return fail(AOG_ERR_INVALID, "aog_lqg_update: no gains (aog_lqg_solve has not run since the last aog_lqg_set_model)");
  HIP_TRY(hipSetDevice(g->state.device));
  const int epb = 256 / g->cfg.act_dim;   // whole envs per workgroup (act_dim <= 128: at least 2)
  const dim3 grid((unsigned)((g->cfg.num_envs + epb - 1) / epb));
  with_models(g->cfg.n_models, [&](auto S) {
    hipLaunchKernelGGL(aog::k_lqg_update<S()>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), records(g), y_dev, out_dev, mask_dev,
                       g->cfg.num_envs, g->cfg.act_dim, epb);
  });
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_lqg_reset(aog_lqg* g, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_lqg_reset", {"lqg", g});
  LAUNCH_PLAIN(g->state.device, stream, aog::k_lqg_reset, grid_of(g), dim3(256), records(g), mask_dev, g->cfg.num_envs, g->cfg.act_dim, g->cfg.n_models);
  return AOG_OK;
}

int64_t aog_lqg_state_bytes(const aog_lqg* g) { return handle_state_bytes(g); }

int aog_lqg_get_state(aog_lqg* g, void* blob_dev, void* stream) { return handle_get_state("aog_lqg_get_state", "lqg", g, blob_dev, stream); }

int aog_lqg_set_state(aog_lqg* g, const void* blob_dev, void* stream) {
  if (int rc = handle_set_state("aog_lqg_set_state", "lqg", g, blob_dev, stream)) return rc;
  // whether the blob holds gains comes back from the device: the one wait of this handle's calls
  LAUNCH_PLAIN(g->state.device, stream, aog::k_lqg_all_solved, dim3(1), dim3(256), (const double*)records(g), g->all_solved, g->cfg.num_envs,
               g->cfg.act_dim, g->cfg.n_models);
  int all = 0;
  HIP_TRY(hipMemcpyAsync(&all, g->all_solved, sizeof all, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  g->solved = all != 0;
  return AOG_OK;
}

}  // extern "C"
