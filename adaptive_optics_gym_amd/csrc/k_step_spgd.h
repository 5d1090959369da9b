// SPGD stepping (aog_reset_spgd / aog_step_spgd): the epilogue of step t, the SPGD query on its metric and the prologue of step t + 1 as one
// launch.
#pragma once
#include "k_spgd.h"
#include "k_step.h"

namespace aog {

// ------------------------------------------------------------------------------------------------
// k_epilogue_spgd_prologue: the fused step tail of aog_reset_spgd / aog_step_spgd, structured like k_epilogue_act_prologue (k_step_act.h).
// Workgroup b (1024 threads = 16 waves) owns envs [16 b, 16 b + 16) in all three phases:
//   1. epilogue_body over the padded batch;
//   2. the SPGD query of those 16 envs, one wave each, on the float32 metric the epilogue has just stored (power, Strehl or reward: s.metric
//      points into the step's own output, written by this workgroup's wave 0 and read after the barrier); the commands go to global memory;
//   3. prologue_body_lds for step t + 1 from those commands.
// The query needs no LDS; the launch's dynamic LDS is the larger of the epilogue's and the prologue's.  Its cost is the launch and three
// dependent memory round trips (metric, record, commands), not bandwidth: 8 (A + 2) bytes of state per env each way.
// ------------------------------------------------------------------------------------------------
constexpr int kStepSpgdThreads = 1024;
static_assert(kStepSpgdThreads / 64 == kEpiEnvs, "one query wave and one prologue wave per env of the workgroup");
__host__ __device__ inline size_t step_spgd_lds_bytes(size_t epi_bytes) {
  const size_t pro = (size_t)prologue_lds_doubles<true, kEpiEnvs>() * sizeof(double);
  return epi_bytes > pro ? epi_bytes : pro;
}
template <bool DET>
__device__ __forceinline__ void step_spgd_body(const EpilogueArgs& p, const SpgdArgs& s, const PrologueArgs& q, const DetectorArgs* d, double* sm) {
  const int block = (int)blockIdx.x;
  const int env0 = block * kEpiEnvs;
  epilogue_body<DET>(p, block, sm, d);
  __syncthreads();
  if (env0 >= s.B) return;   // (uniform per workgroup: the padding past B runs the epilogue only)
  const int env = env0 + (int)(threadIdx.x >> 6);
  if (env < s.B) spgd_query(s, env, (int)(threadIdx.x & 63));
  __syncthreads();   // the commands are written and the epilogue's LDS is free
  prologue_body_lds<true, kEpiEnvs>(q, block, sm, sm + 64 * 64);
}
__global__ __launch_bounds__(kStepSpgdThreads) void k_epilogue_spgd_prologue(EpilogueArgs p, SpgdArgs s, PrologueArgs q) {
  extern __shared__ double sm[];
  step_spgd_body<false>(p, s, q, nullptr, sm);
}
// for handles with a detector: the metric is the clean power, Strehl or reward; only the observation is noisy
__global__ __launch_bounds__(kStepSpgdThreads) void k_epilogue_spgd_prologue_det(EpilogueArgs p, SpgdArgs s, PrologueArgs q, DetectorArgs d) {
  extern __shared__ double sm[];
  step_spgd_body<true>(p, s, q, &d, sm);
}

}  // namespace aog
