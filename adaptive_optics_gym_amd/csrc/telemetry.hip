// K18: closed-loop modal telemetry (aog_telemetry_*): per-env rings of measurements, their Welch PSDs and the optimised integrator gains.
// Independent of any aog_env.
#include "standalone_handle.h"
#include "k_telemetry.h"

using namespace aog_host;

struct aog_telemetry : StandaloneHandle<aog_telemetry_config> {   // state: [batch] records (k_telemetry.h)
  size_t rec_bytes = 0;
  double* r2 = nullptr;    // |R_k(g)|^2 of the last aog_telemetry_gains and its grid: kTelMaxG (kTelMaxT / 2 + 1) float64
};

namespace {

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int telemetry_check(const aog_telemetry_config* c) {
  if (c->batch < 1 || c->act_dim < 1 || c->act_dim > aog::kTelMaxA)
    return fail(AOG_ERR_INVALID, "aog_telemetry_create: bad dimensions (batch %d, act_dim %d; act_dim <= %d)", c->batch, c->act_dim, aog::kTelMaxA);
  if (!pow2(c->length) || c->length < aog::kTelMinT || c->length > aog::kTelMaxT)
    return fail(AOG_ERR_INVALID, "aog_telemetry_create: length %d must be a power of two in [%d, %d]", c->length, aog::kTelMinT, aog::kTelMaxT);
  return AOG_OK;
}

int segment_check(const aog_telemetry* t, const char* who, int S) {
  if (!pow2(S) || S < aog::kTelMinS || S > t->cfg.length)
    return fail(AOG_ERR_INVALID, "%s: segment %d must be a power of two in [%d, length %d]", who, S, aog::kTelMinS, t->cfg.length);
  return AOG_OK;
}

aog::TelemetryArgs telemetry_args(const aog_telemetry* t, const uint8_t* mask) {
  aog::TelemetryArgs a{};
  a.state = t->state.ptr;
  a.rec_bytes = t->rec_bytes;
  a.mask = mask;
  a.A = t->cfg.act_dim;
  a.T = t->cfg.length;
  return a;
}

template <int S>
int launch_psd(const aog_telemetry* t, const aog::TelemetryArgs& a, hipStream_t s) {
  using Geo = aog::TelGeom<S>;
  const int nmb = (a.A + Geo::M - 1) / Geo::M;
  return launch_with_lds(t->state.device, s, aog::k_telemetry_psd<S>, dim3((unsigned)t->cfg.batch * nmb), dim3(aog::kTelThreads), Geo::kLdsWords * sizeof(double), a);
}

int launch_psd_for(const aog_telemetry* t, int S, const aog::TelemetryArgs& a, hipStream_t s) {
  switch (S) {
    case 32: return launch_psd<32>(t, a, s);
    case 64: return launch_psd<64>(t, a, s);
    case 128: return launch_psd<128>(t, a, s);
    case 256: return launch_psd<256>(t, a, s);
    case 512: return launch_psd<512>(t, a, s);
    default: return launch_psd<1024>(t, a, s);
  }
}

// the stability limit of z^d - z^(d-1) + g = 0: 2 at d = 1, 1 at d = 2
double gain_limit(int delay) { return 2.0 * std::sin(M_PI / (2.0 * (2.0 * delay - 1.0))); }

}  // namespace

extern "C" {

int aog_telemetry_create(const aog_telemetry_config* cfg, int device, aog_telemetry** out) {
  return handle_create("aog_telemetry_create", cfg, device, out, telemetry_check, [](aog_telemetry* t) {
    t->rec_bytes = aog::telemetry_record_words(t->cfg.act_dim, t->cfg.length) * sizeof(double);
    if (hipError_t err = t->alloc_state(t->rec_bytes * (size_t)t->cfg.batch, false)) return err;
    if (hipError_t err = t->own(&t->r2, sizeof(double) * aog::kTelMaxG * (aog::kTelMaxT / 2 + 1), false)) return err;
    hipLaunchKernelGGL(aog::k_telemetry_reset, dim3(t->cfg.batch), dim3(256), 0, nullptr, telemetry_args(t, nullptr));
    return hipGetLastError();
  });
}

void aog_telemetry_destroy(aog_telemetry* t) { handle_destroy(t); }

int aog_telemetry_reset(aog_telemetry* t, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_telemetry_reset", {"t", t});
  LAUNCH_PLAIN(t->state.device, stream, aog::k_telemetry_reset, dim3(t->cfg.batch), dim3(256), telemetry_args(t, mask_dev));
  return AOG_OK;
}

int aog_telemetry_push(aog_telemetry* t, const double* y_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_telemetry_push", {"t", t}, {"y_dev", y_dev});
  aog::TelemetryArgs a = telemetry_args(t, mask_dev);
  a.y = y_dev;
  LAUNCH_PLAIN(t->state.device, stream, aog::k_telemetry_push, dim3(t->cfg.batch), dim3(aog::kTelMaxA), a);
  return AOG_OK;
}

int aog_telemetry_psd(aog_telemetry* t, int segment, double* psd_dev, int32_t* segments_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_telemetry_psd", {"t", t}, {"psd_dev", psd_dev});
  if (int rc = segment_check(t, "aog_telemetry_psd", segment)) return rc;
  HIP_TRY(hipSetDevice(t->state.device));
  aog::TelemetryArgs a = telemetry_args(t, mask_dev);
  a.psd = psd_dev;
  a.segments = segments_dev;
  return launch_psd_for(t, segment, a, static_cast<hipStream_t>(stream));
}

int aog_telemetry_gains(aog_telemetry* t, int segment, int delay, const double* grid_host, int n_grid, double* gain_dev, double* cost_dev,
                        double* cost_all_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_telemetry_gains", {"t", t}, {"grid_host", grid_host}, {"gain_dev", gain_dev}, {"cost_dev", cost_dev});
  if (int rc = segment_check(t, "aog_telemetry_gains", segment)) return rc;
  if (delay < 1 || delay > aog::kTelMaxDelay) return fail(AOG_ERR_INVALID, "aog_telemetry_gains: delay %d outside [1, %d]", delay, aog::kTelMaxDelay);
  if (n_grid < 1 || n_grid > aog::kTelMaxG) return fail(AOG_ERR_INVALID, "aog_telemetry_gains: %d candidates outside [1, %d]", n_grid, aog::kTelMaxG);
  const double g_max = gain_limit(delay);
  aog::TelemetryRkArgs rk{};
  for (int i = 0; i < n_grid; ++i) {
    const double g = grid_host[i];
    if (!(g > 0.0 && g < g_max))
      return fail(AOG_ERR_INVALID, "aog_telemetry_gains: candidate %d = %g outside (0, %g), the stable gains of an integrator with delay %d", i, g, g_max, delay);
    if (i && !(g > grid_host[i - 1])) return fail(AOG_ERR_INVALID, "aog_telemetry_gains: the grid must ascend (candidate %d = %g after %g)", i, g, grid_host[i - 1]);
    rk.grid[i] = g;
  }
  rk.r2 = t->r2;
  rk.S = segment;
  rk.G = n_grid;
  rk.delay = delay;
  LAUNCH_PLAIN(t->state.device, stream, aog::k_telemetry_rk, dim3((segment / 2 + 255) / 256, n_grid), dim3(256), rk);
  aog::TelemetryArgs a = telemetry_args(t, mask_dev);
  a.r2 = t->r2;
  a.gain = gain_dev;
  a.cost = cost_dev;
  a.cost_all = cost_all_dev;
  a.G = n_grid;
  return launch_psd_for(t, segment, a, static_cast<hipStream_t>(stream));
}

int64_t aog_telemetry_state_bytes(const aog_telemetry* t) { return handle_state_bytes(t); }

int aog_telemetry_get_state(aog_telemetry* t, void* blob_dev, void* stream) {
  return handle_get_state("aog_telemetry_get_state", "t", t, blob_dev, stream);
}

int aog_telemetry_set_state(aog_telemetry* t, const void* blob_dev, void* stream) {
  return handle_set_state("aog_telemetry_set_state", "t", t, blob_dev, stream);
}

}  // extern "C"
