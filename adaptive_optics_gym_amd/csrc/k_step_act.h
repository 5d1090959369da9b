// Causal policy stepping (aog_reset_act / aog_step_act): the epilogue of step t, the policy query on its observation and the prologue of
// step t + 1 as one launch.
#pragma once
#include "k_actor.h"
#include "k_step.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// R2  k_epilogue_act_prologue.  Workgroup b (1024 threads) owns envs [16 b, 16 b + 16) in all three phases, so no phase waits for another
// workgroup:
//   1. epilogue_body (k_epilogue's code) over the padded batch: obs, obs_raw, reward, done, power, Strehl, return accumulator;
//   2. the four layers of k_actor_act (actor_mlp) on those 16 observations, float16 widened to float as DeviceActor sees them: taken from the
//      epilogue's powers in LDS on the table route, read from global memory on the separable route (k_obs_pass2 wrote them earlier on the
//      stream); action / log_prob / mean to the caller's buffers;
//   3. prologue_body for step t + 1 from the actions just written (global memory, made visible to the workgroup by the barrier).
// Each output tile of an actor layer is the same chain of v_mfma_f32_16x16x4f32 whatever wave runs it, and the prologue's float64 arithmetic
// does not depend on the launch shape: the results are those of k_epilogue + k_actor_act + k_prologue bit for bit (log_prob up to the
// order of its LDS atomics, as in k_actor_act).  The phases run one after the other, so they share one dynamic LDS allocation
// (step_act_lds_bytes = the largest of the three).  Layer 1's first weight chunk is requested before the epilogue's slab reduction and
// travels while it runs.
// ------------------------------------------------------------------------------------------------
constexpr int kStepActThreads = 1024;
constexpr int kStepActPre = 6;   // 1024 x 6 x 4 = kActorWFloats
static_assert(kStepActThreads * kStepActPre * 4 >= kActorWFloats, "a weight chunk must fit the registers in flight");
static_assert(kStepActThreads / 64 == kEpiEnvs && kEpiEnvs == 16, "one prologue wave per env of the workgroup, 16 envs per actor tile");
constexpr int kStepActProDoubles = prologue_lds_doubles<true, kEpiEnvs>();
__host__ __device__ inline size_t step_act_lds_bytes(size_t epi_bytes, size_t actor_bytes) {
  const size_t pro = (size_t)kStepActProDoubles * sizeof(double);
  return epi_bytes > actor_bytes ? (epi_bytes > pro ? epi_bytes : pro) : (actor_bytes > pro ? actor_bytes : pro);
}

// obs_from_lds: table route (the observation is the epilogue's pw[0 .. S)); otherwise a.obs holds float16 observations [B][S]
__global__ __launch_bounds__(kStepActThreads) void k_epilogue_act_prologue(EpilogueArgs p, ActorArgs a, PrologueArgs q, int obs_from_lds) {
  extern __shared__ double sm[];
  const int block = (int)blockIdx.x;
  const int env0 = block * kEpiEnvs;
  const bool act = env0 < a.B;   // (uniform per workgroup: the padding past B runs the epilogue only)
  f32x4 pre[kStepActPre];
  if (act) actor_issue<kStepActThreads, kStepActPre>(pre, a.w1, a.S, a.H, 0, a.wfloats);
  epilogue_body(p, block, sm);
  __syncthreads();
  if (!act) return;
  // table route: this thread's element of the staged observations (k = i / 16, env e = i % 16; S * 16 <= 49 * 16 < 1024) out of the
  // epilogue's LDS before the activations overwrite it, rounded to float16 exactly as the epilogue stored it
  float ov = 0.f;
  const int i = threadIdx.x;
  if (obs_from_lds && i < a.S * 16) {
    const double w = sm[EpilogueLds(p).pw + i];
    ov = (float)(_Float16)w;
  }
  __syncthreads();
  float* lds_act = reinterpret_cast<float*>(sm);
  float* xa = lds_act;
  for (int j = threadIdx.x; j < (int)actor_act_floats(a.kpad, a.kpad_b); j += kStepActThreads) lds_act[j] = 0.f;
  __syncthreads();
  if (obs_from_lds) {
    if (i < a.S * 16) xa[i] = ov;
  } else {
    const _Float16* obs = reinterpret_cast<const _Float16*>(a.obs);
    for (int j = threadIdx.x; j < a.S * 16; j += kStepActThreads) {
      const int k = j >> 4, e = j & 15, env = min(env0 + e, a.B - 1);
      xa[j] = (float)obs[(size_t)env * a.S + k];
    }
  }
  __syncthreads();
  actor_mlp<kStepActThreads, kStepActPre>(a, lds_act, env0, pre);   // (ends with a barrier: the actions are written and the LDS is free)
  prologue_body_lds<true, kEpiEnvs>(q, block, sm, sm + 64 * 64);
}

// k_epilogue_act_prologue with the query's action form a.nz (aog_reset_act_noise / aog_step_act_noise: mean mode and / or an OU term), as in
// k_actor_act_noise.  A kernel of its own, the body above repeated: the plain kernel keeps its arguments and code (a shared body changes its
// register allocation; see profiles/action_noise.md).
__global__ __launch_bounds__(kStepActThreads) void k_epilogue_act_prologue_noise(EpilogueArgs p, ActorNoiseArgs a, PrologueArgs q, int obs_from_lds) {
  extern __shared__ double sm[];
  const int block = (int)blockIdx.x;
  const int env0 = block * kEpiEnvs;
  const bool act = env0 < a.B;   // (uniform per workgroup: the padding past B runs the epilogue only)
  f32x4 pre[kStepActPre];
  if (act) actor_issue<kStepActThreads, kStepActPre>(pre, a.w1, a.S, a.H, 0, a.wfloats);
  epilogue_body(p, block, sm);
  __syncthreads();
  if (!act) return;
  // table route: this thread's element of the staged observations (k = i / 16, env e = i % 16; S * 16 <= 49 * 16 < 1024) out of the
  // epilogue's LDS before the activations overwrite it, rounded to float16 exactly as the epilogue stored it
  float ov = 0.f;
  const int i = threadIdx.x;
  if (obs_from_lds && i < a.S * 16) {
    const double w = sm[EpilogueLds(p).pw + i];
    ov = (float)(_Float16)w;
  }
  __syncthreads();
  float* lds_act = reinterpret_cast<float*>(sm);
  float* xa = lds_act;
  for (int j = threadIdx.x; j < (int)actor_act_floats(a.kpad, a.kpad_b); j += kStepActThreads) lds_act[j] = 0.f;
  __syncthreads();
  if (obs_from_lds) {
    if (i < a.S * 16) xa[i] = ov;
  } else {
    const _Float16* obs = reinterpret_cast<const _Float16*>(a.obs);
    for (int j = threadIdx.x; j < a.S * 16; j += kStepActThreads) {
      const int k = j >> 4, e = j & 15, env = min(env0 + e, a.B - 1);
      xa[j] = (float)obs[(size_t)env * a.S + k];
    }
  }
  __syncthreads();
  actor_mlp<kStepActThreads, kStepActPre, true, ActorNoiseArgs>(a, lds_act, env0, pre);   // (ends with a barrier: the actions are written and the LDS is free)
  prologue_body_lds<true, kEpiEnvs>(q, block, sm, sm + 64 * 64);
}

// The two kernels above for handles with a detector (aog_set_detector): epilogue_body<true> draws the noisy observation, and the table route
// stages the actor's input from the noisy plane pwn — the float16 that was stored.  Kernels of their own, so that the plain ones keep their
// arguments and code.
template <bool NOISE, class A>
__device__ __forceinline__ void step_act_det_body(const EpilogueArgs& p, const A& a, const PrologueArgs& q, int obs_from_lds, const DetectorArgs& d,
                                                  double* sm) {
  const int block = (int)blockIdx.x;
  const int env0 = block * kEpiEnvs;
  const bool act = env0 < a.B;   // (uniform per workgroup: the padding past B runs the epilogue only)
  f32x4 pre[kStepActPre];
  if (act) actor_issue<kStepActThreads, kStepActPre>(pre, a.w1, a.S, a.H, 0, a.wfloats);
  epilogue_body<true>(p, block, sm, &d);
  __syncthreads();
  if (!act) return;
  float ov = 0.f;
  const int i = threadIdx.x;
  if (obs_from_lds && i < a.S * 16) {
    const double y = sm[EpilogueLds(p, true).pwn + i];
    ov = (float)(_Float16)y;
  }
  __syncthreads();
  float* lds_act = reinterpret_cast<float*>(sm);
  float* xa = lds_act;
  for (int j = threadIdx.x; j < (int)actor_act_floats(a.kpad, a.kpad_b); j += kStepActThreads) lds_act[j] = 0.f;
  __syncthreads();
  if (obs_from_lds) {
    if (i < a.S * 16) xa[i] = ov;
  } else {
    const _Float16* obs = reinterpret_cast<const _Float16*>(a.obs);
    for (int j = threadIdx.x; j < a.S * 16; j += kStepActThreads) {
      const int k = j >> 4, e = j & 15, env = min(env0 + e, a.B - 1);
      xa[j] = (float)obs[(size_t)env * a.S + k];
    }
  }
  __syncthreads();
  actor_mlp<kStepActThreads, kStepActPre, NOISE, A>(a, lds_act, env0, pre);   // (ends with a barrier: the actions are written and the LDS is free)
  prologue_body_lds<true, kEpiEnvs>(q, block, sm, sm + 64 * 64);
}
__global__ __launch_bounds__(kStepActThreads) void k_epilogue_act_prologue_det(EpilogueArgs p, ActorArgs a, PrologueArgs q, int obs_from_lds,
                                                                               DetectorArgs d) {
  extern __shared__ double sm[];
  step_act_det_body<false, ActorArgs>(p, a, q, obs_from_lds, d, sm);
}
__global__ __launch_bounds__(kStepActThreads) void k_epilogue_act_prologue_noise_det(EpilogueArgs p, ActorNoiseArgs a, PrologueArgs q, int obs_from_lds,
                                                                                     DetectorArgs d) {
  extern __shared__ double sm[];
  step_act_det_body<true, ActorNoiseArgs>(p, a, q, obs_from_lds, d, sm);
}

}  // namespace aog
