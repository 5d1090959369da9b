// The SPGD controller's handle (aog_spgd), shared by spgd.hip (its own entry points) and aogym.hip (aog_reset_spgd / aog_step_spgd).
#pragma once
#include "standalone_handle.h"
#include "k_spgd.h"

struct aog_spgd : aog_host::StandaloneHandle<aog_spgd_config> {   // state: [B] records (k_spgd.h)
  double* gain = nullptr;        // [B]
  double* amplitude = nullptr;   // [B]
  float* metric = nullptr;       // [B] where a fused step stores the metric when the caller passes no output for it
};

namespace aog_host {
// the arguments of one query (reset = false: on `metric`) or reset (from `start`, nullable) writing the commands to `action`
inline aog::SpgdArgs spgd_args(const aog_spgd* g, bool reset, const float* metric, const uint8_t* mask, const double* start, float* action) {
  aog::SpgdArgs s{};
  s.state = reinterpret_cast<double*>(g->state.ptr);
  s.gain = g->gain;
  s.amplitude = g->amplitude;
  s.metric = metric;
  s.mask = mask;
  s.start = start;
  s.action = action;
  s.B = g->cfg.num_envs;
  s.A = g->cfg.act_dim;
  s.env_base = g->cfg.env_id_base;
  s.reset = reset ? 1 : 0;
  s.seed_lo = (uint32_t)g->cfg.seed;
  s.seed_hi = (uint32_t)(g->cfg.seed >> 32);
  s.clip = g->cfg.clip;
  return s;
}
}  // namespace aog_host
