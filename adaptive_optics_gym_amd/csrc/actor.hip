// R1: policy query kernel (aog_actor_act) and the argument checks it shares with the fused step tail (aog_step_act).
#include "host_common.h"
#include "k_actor.h"

using namespace aog_host;

namespace aog {
__global__ __launch_bounds__(kActorThreads) void k_actor_act(ActorArgs p) {
  extern __shared__ float lds_act[];   // actor_mlp's layout
  float* xa = lds_act;
  const int env0 = blockIdx.x * 16;
  f32x4 pre[kActorPre];
  actor_issue<kActorThreads, kActorPre>(pre, p.w1, p.S, p.H, 0, p.wfloats);   // the first weight chunk travels while the observations are staged
  for (int i = threadIdx.x; i < (int)actor_act_floats(p.kpad, p.kpad_b); i += kActorThreads) lds_act[i] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < p.S * 16; i += kActorThreads) {
    const int k = i >> 4, e = i & 15, env = min(env0 + e, p.B - 1);
    xa[i] = p.obs_f16 ? (float)reinterpret_cast<const _Float16*>(p.obs)[(size_t)env * p.S + k]
                      : reinterpret_cast<const float*>(p.obs)[(size_t)env * p.S + k];
  }
  __syncthreads();
  actor_mlp<kActorThreads, kActorPre>(p, lds_act, env0, pre);
}
// k_actor_act with an action form (aog_actor_act_noise: mean mode and / or an OU term).  A kernel of its own, with the staging above repeated:
// the plain kernel keeps its arguments and code (a shared body changes its register allocation; see profiles/action_noise.md).
__global__ __launch_bounds__(kActorThreads) void k_actor_act_noise(ActorNoiseArgs p) {
  extern __shared__ float lds_act[];   // actor_mlp's layout
  float* xa = lds_act;
  const int env0 = blockIdx.x * 16;
  f32x4 pre[kActorPre];
  actor_issue<kActorThreads, kActorPre>(pre, p.w1, p.S, p.H, 0, p.wfloats);   // the first weight chunk travels while the observations are staged
  for (int i = threadIdx.x; i < (int)actor_act_floats(p.kpad, p.kpad_b); i += kActorThreads) lds_act[i] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < p.S * 16; i += kActorThreads) {
    const int k = i >> 4, e = i & 15, env = min(env0 + e, p.B - 1);
    xa[i] = p.obs_f16 ? (float)reinterpret_cast<const _Float16*>(p.obs)[(size_t)env * p.S + k]
                      : reinterpret_cast<const float*>(p.obs)[(size_t)env * p.S + k];
  }
  __syncthreads();
  actor_mlp<kActorThreads, kActorPre, true, ActorNoiseArgs>(p, lds_act, env0, pre);
}
}  // namespace aog

namespace aog_host {
// aog_actor_act's checks and arguments (everything but the observations and outputs); *lds = its dynamic LDS: the activations and one weight
// chunk, which takes what the activations leave of the LDS, at most kActorWFloats, and must hold one 16-row tile of the widest layer
// (state_dim 1024 = the 32 x 32 observation: 64 KB of observations beside the chunk)
int actor_args(const aog_actor* n, const char* who, aog::ActorArgs* out, size_t* lds) {
  if (!n) return fail(AOG_ERR_INVALID, "%s: null argument", who);
  if (n->batch < 0 || n->state_dim < 1 || n->hidden_dim < 1 || n->act_dim < 1 || n->hidden_dim > 1024 || n->state_dim > 1024 || n->act_dim > 4096)
    return fail(AOG_ERR_INVALID, "%s: bad dimensions (batch %d, state %d, hidden %d, act %d)", who, n->batch, n->state_dim, n->hidden_dim, n->act_dim);
  if (!n->w1 || !n->b1 || !n->w2 || !n->b2 || !n->w3 || !n->b3 || !n->wo || !n->bo) return fail(AOG_ERR_INVALID, "%s: null weight pointer", who);
  if (((uintptr_t)n->w1 | (uintptr_t)n->w2 | (uintptr_t)n->w3 | (uintptr_t)n->wo) & 15) return fail(AOG_ERR_INVALID, "%s: weight matrices must be 16-byte aligned", who);
  if (!(n->dropout_p >= 0.f && n->dropout_p < 1.f) || !(n->cov_var > 0.f)) return fail(AOG_ERR_INVALID, "%s: dropout_p must be in [0,1), cov_var > 0", who);
  aog::ActorArgs a{};
  a.w1 = n->w1; a.b1 = n->b1; a.w2 = n->w2; a.b2 = n->b2; a.w3 = n->w3; a.b3 = n->b3; a.wo = n->wo; a.bo = n->bo;
  a.B = n->batch; a.S = n->state_dim; a.H = n->hidden_dim; a.A = n->act_dim;
  a.kpad = round_up(std::max(n->state_dim, n->hidden_dim), 16);
  a.kpad_b = round_up(n->hidden_dim, 16);
  const size_t act_floats = aog::actor_act_floats(a.kpad, a.kpad_b);
  a.wfloats = (int)std::min<size_t>(aog::kActorWFloats, (kLdsBytes / sizeof(float) - act_floats) / 4 * 4);
  if (a.wfloats < 16 * a.kpad)
    return fail(AOG_ERR_UNSUPPORTED, "%s: state_dim %d with hidden_dim %d does not fit the LDS (activations %zu floats + one 16-row weight tile)", who,
                n->state_dim, n->hidden_dim, act_floats);
  a.p_drop = n->dropout_p;
  a.keep_scale = 1.0f / (1.0f - n->dropout_p);
  a.std = std::sqrt(n->cov_var);
  a.logp_const = 0.5f * (float)n->act_dim * std::log(2.0f * (float)M_PI * n->cov_var);
  a.seed = n->seed;
  a.call_lo = (uint32_t)n->call_index;
  a.call_hi = (uint32_t)(n->call_index >> 32);
  a.env_base = n->env_id_base;
  *out = a;
  *lds = (act_floats + (size_t)a.wfloats) * sizeof(float);
  return AOG_OK;
}

// the checks of an aog_action_noise (NULL: none) and the kernels' form of it; *noisy = the query needs the NOISE instantiation (mean mode
// or an OU term)
int action_noise_args(const aog_action_noise* nz, const char* who, aog::ActorNoise* out, bool* noisy) {
  *out = aog::ActorNoise{0, nullptr, 0.0, 0.0, 0.0};
  *noisy = false;
  if (!nz) return AOG_OK;
  if (nz->mode != AOG_ACTION_SAMPLE && nz->mode != AOG_ACTION_MEAN) return fail(AOG_ERR_INVALID, "%s: action mode %d (0 = sample, 1 = mean)", who, nz->mode);
  if (nz->reserved0 != 0) return fail(AOG_ERR_INVALID, "%s: aog_action_noise.reserved0 must be 0", who);
  if (!std::isfinite(nz->ou_mu) || !std::isfinite(nz->ou_theta) || !std::isfinite(nz->ou_sigma) || nz->ou_sigma < 0.0)
    return fail(AOG_ERR_INVALID, "%s: OU parameters must be finite, ou_sigma >= 0 (mu %g, theta %g, sigma %g)", who, nz->ou_mu, nz->ou_theta, nz->ou_sigma);
  *out = aog::ActorNoise{nz->mode, nz->ou_state, nz->ou_mu, nz->ou_theta, nz->ou_sigma};
  *noisy = nz->mode != AOG_ACTION_SAMPLE || nz->ou_state != nullptr;
  return AOG_OK;
}
}  // namespace aog_host

extern "C" {

int aog_actor_act_noise(const aog_actor* n, int device, const void* obs_dev, int obs_is_f16, float* mean_dev, float* action_dev, float* log_prob_dev,
                        const aog_action_noise* noise, void* stream) {
  if (!n || !obs_dev) return fail(AOG_ERR_INVALID, "aog_actor_act: null argument");
  aog::ActorNoise nz{};
  bool noisy = false;
  if (int rc = action_noise_args(noise, "aog_actor_act", &nz, &noisy)) return rc;
  aog::ActorArgs a{};
  size_t lds = 0;
  if (int rc = actor_args(n, "aog_actor_act", &a, &lds)) return (rc == AOG_ERR_UNSUPPORTED && n->batch == 0) ? AOG_OK : rc;   // (nothing to launch)
  if (n->batch == 0) return AOG_OK;
  HIP_TRY(hipSetDevice(device));
  a.obs = obs_dev;
  a.obs_f16 = obs_is_f16 ? 1 : 0;
  a.mean = mean_dev; a.action = action_dev; a.log_prob = log_prob_dev;
  const void* kernel = noisy ? reinterpret_cast<const void*>(aog::k_actor_act_noise) : reinterpret_cast<const void*>(aog::k_actor_act);
  if (int rc = aog_host::ensure_dynamic_lds(kernel, lds, device)) return rc;
  const dim3 grid((n->batch + 15) / 16), block(aog::kActorThreads);
  if (noisy) hipLaunchKernelGGL(aog::k_actor_act_noise, grid, block, lds, static_cast<hipStream_t>(stream), aog::ActorNoiseArgs{a, nz});
  else hipLaunchKernelGGL(aog::k_actor_act, grid, block, lds, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_actor_act(const aog_actor* n, int device, const void* obs_dev, int obs_is_f16, float* mean_dev, float* action_dev, float* log_prob_dev,
                  void* stream) {
  return aog_actor_act_noise(n, device, obs_dev, obs_is_f16, mean_dev, action_dev, log_prob_dev, nullptr, stream);
}

}  // extern "C"
