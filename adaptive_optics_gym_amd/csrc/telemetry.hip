// K18: closed-loop modal telemetry (aog_telemetry_*): per-env rings of measurements, their Welch PSDs and the optimised integrator gains.
// Independent of any aog_env.
#include "host_common.h"
#include "k_telemetry.h"

using namespace aog_host;

struct aog_telemetry {
  aog_telemetry_config cfg{};
  size_t rec_bytes = 0;
  RecordStore state;       // [batch] records (k_telemetry.h)
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

void release(aog_telemetry* t) {
  t->state.release();
  if (t->r2) (void)hipFree(t->r2);
  delete t;
}

// the stability limit of z^d - z^(d-1) + g = 0: 2 at d = 1, 1 at d = 2
double gain_limit(int delay) { return 2.0 * std::sin(M_PI / (2.0 * (2.0 * delay - 1.0))); }

}  // namespace

extern "C" {

int aog_telemetry_create(const aog_telemetry_config* cfg, int device, aog_telemetry** out) {
  if (!cfg || !out) return fail(AOG_ERR_INVALID, "aog_telemetry_create: null argument");
  *out = nullptr;
  if (int rc = telemetry_check(cfg)) return rc;
  HIP_TRY(hipSetDevice(device));
  aog_telemetry* t = new aog_telemetry;
  t->cfg = *cfg;
  t->rec_bytes = aog::telemetry_record_words(cfg->act_dim, cfg->length) * sizeof(double);
  hipError_t err = t->state.alloc(device, t->rec_bytes * (size_t)cfg->batch);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&t->r2), sizeof(double) * aog::kTelMaxG * (aog::kTelMaxT / 2 + 1));
  if (err == hipSuccess) {
    hipLaunchKernelGGL(aog::k_telemetry_reset, dim3(cfg->batch), dim3(256), 0, nullptr, telemetry_args(t, nullptr));
    err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  }
  if (err != hipSuccess) {
    release(t);
    return fail(AOG_ERR_HIP, "aog_telemetry_create: %s", hipGetErrorString(err));
  }
  *out = t;
  return AOG_OK;
}

void aog_telemetry_destroy(aog_telemetry* t) {
  if (!t) return;
  (void)hipSetDevice(t->state.device);
  release(t);
}

int aog_telemetry_reset(aog_telemetry* t, const uint8_t* mask_dev, void* stream) {
  if (!t) return fail(AOG_ERR_INVALID, "aog_telemetry_reset: null argument");
  LAUNCH_PLAIN(t->state.device, stream, aog::k_telemetry_reset, dim3(t->cfg.batch), dim3(256), telemetry_args(t, mask_dev));
  return AOG_OK;
}

int aog_telemetry_push(aog_telemetry* t, const double* y_dev, const uint8_t* mask_dev, void* stream) {
  if (!t || !y_dev) return fail(AOG_ERR_INVALID, "aog_telemetry_push: null argument");
  aog::TelemetryArgs a = telemetry_args(t, mask_dev);
  a.y = y_dev;
  LAUNCH_PLAIN(t->state.device, stream, aog::k_telemetry_push, dim3(t->cfg.batch), dim3(aog::kTelMaxA), a);
  return AOG_OK;
}

int aog_telemetry_psd(aog_telemetry* t, int segment, double* psd_dev, int32_t* segments_dev, const uint8_t* mask_dev, void* stream) {
  if (!t || !psd_dev) return fail(AOG_ERR_INVALID, "aog_telemetry_psd: null argument");
  if (int rc = segment_check(t, "aog_telemetry_psd", segment)) return rc;
  HIP_TRY(hipSetDevice(t->state.device));
  aog::TelemetryArgs a = telemetry_args(t, mask_dev);
  a.psd = psd_dev;
  a.segments = segments_dev;
  return launch_psd_for(t, segment, a, static_cast<hipStream_t>(stream));
}

int aog_telemetry_gains(aog_telemetry* t, int segment, int delay, const double* grid_host, int n_grid, double* gain_dev, double* cost_dev,
                        double* cost_all_dev, const uint8_t* mask_dev, void* stream) {
  if (!t || !grid_host || !gain_dev || !cost_dev) return fail(AOG_ERR_INVALID, "aog_telemetry_gains: null argument");
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

int64_t aog_telemetry_state_bytes(const aog_telemetry* t) { return t ? (int64_t)t->state.bytes : 0; }

int aog_telemetry_get_state(aog_telemetry* t, void* blob_dev, void* stream) {
  if (!t || !blob_dev) return fail(AOG_ERR_INVALID, "aog_telemetry_get_state: null argument");
  return t->state.copy_out(blob_dev, stream);
}

int aog_telemetry_set_state(aog_telemetry* t, const void* blob_dev, void* stream) {
  if (!t || !blob_dev) return fail(AOG_ERR_INVALID, "aog_telemetry_set_state: null argument");
  return t->state.copy_in(blob_dev, stream);
}

}  // extern "C"
