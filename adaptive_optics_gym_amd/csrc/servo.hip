// K22: the mirror servo (aog_servo_*): loop latency, first-order mirror response, finite stroke and stuck actuators between the commanded
// action and the action the mirror receives.  Independent of any aog_env; whoever owns the handle steps the env with what it writes.
#include "host_common.h"
#include <initializer_list>
#include <utility>
#include "k_servo.h"
#include "../../include/aogym_servo.h"

using namespace aog_host;

struct aog_servo {
  aog_servo_config cfg{};
  RecordStore state;            // y [B][A] float64, counter (uint64), ring [B][R][A] float32 (k_servo.h)
  char* params = nullptr;       // frac, response, stroke [B] float64 each | stuck_value [B][A] float32 | delay [B] int32 | stuck [B][A] uint8
  unsigned long long calls = 0; // the counter, kept here: every aog_servo_apply hands n mod R and n + 1 to its launch
};

namespace {

size_t envs(const aog_servo* g) { return (size_t)g->cfg.num_envs; }
size_t cells(const aog_servo* g) { return envs(g) * g->cfg.act_dim; }
int depth(const aog_servo* g) { return g->cfg.max_latency + 2; }
size_t counter_offset(const aog_servo* g) { return sizeof(double) * cells(g); }
size_t param_bytes(const aog_servo* g) { return (3 * sizeof(double) + sizeof(int32_t)) * envs(g) + (sizeof(float) + 1) * cells(g); }

// the parameter block as it goes to the device: the identity until aog_servo_set_params
struct HostParams {
  std::vector<char> bytes;
  double *frac, *response, *stroke;
  float* stuck_value;
  int32_t* delay;
  uint8_t* stuck;
  explicit HostParams(const aog_servo* g) : bytes(param_bytes(g), 0) {
    const size_t B = envs(g), n = cells(g);
    frac = reinterpret_cast<double*>(bytes.data());
    response = frac + B;
    stroke = response + B;
    stuck_value = reinterpret_cast<float*>(stroke + B);
    delay = reinterpret_cast<int32_t*>(stuck_value + n);
    stuck = reinterpret_cast<uint8_t*>(delay + B);
  }
};

aog::ServoArgs servo_args(const aog_servo* g, const float* in, const uint8_t* mask, float* out) {
  const size_t B = envs(g), n = cells(g);
  aog::ServoArgs a{};
  a.y = reinterpret_cast<double*>(g->state.ptr);
  a.counter = reinterpret_cast<unsigned long long*>(g->state.ptr + counter_offset(g));
  a.ring = reinterpret_cast<float*>(g->state.ptr + counter_offset(g) + sizeof(unsigned long long));
  a.frac = reinterpret_cast<const double*>(g->params);
  a.response = a.frac + B;
  a.stroke = a.response + B;
  a.stuck_value = reinterpret_cast<const float*>(a.stroke + B);
  a.delay = reinterpret_cast<const int*>(a.stuck_value + n);
  a.stuck = reinterpret_cast<const uint8_t*>(a.delay + B);
  a.in = in;
  a.mask = mask;
  a.out = out;
  a.B = g->cfg.num_envs;
  a.A = g->cfg.act_dim;
  a.R = depth(g);
  a.slot = (int)(g->calls % (unsigned long long)depth(g));
  a.next = g->calls + 1;
  return a;
}

dim3 grid_of(const aog_servo* g) { return dim3((unsigned)((cells(g) + 255) / 256)); }

// the first null pointer among an entry point's arguments, by name (nullptr: none is null)
const char* first_null(std::initializer_list<std::pair<const char*, const void*>> args) {
  for (const auto& a : args)
    if (!a.second) return a.first;
  return nullptr;
}
#define REFUSE_NULL(who, ...)                                                                      \
  do {                                                                                             \
    if (const char* name__ = first_null({__VA_ARGS__})) return fail(AOG_ERR_INVALID, who ": null argument %s", name__); \
  } while (0)

void release(aog_servo* g) {
  g->state.release();
  if (g->params) (void)hipFree(g->params);
  delete g;
}

}  // namespace

extern "C" {

int64_t aog_servo_config_size(void) { return (int64_t)sizeof(aog_servo_config); }

int aog_servo_create(const aog_servo_config* cfg, int device, aog_servo** out) {
  REFUSE_NULL("aog_servo_create", {"cfg", cfg}, {"out", out});
  *out = nullptr;
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_servo_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_servo_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->act_dim < 1 || cfg->act_dim > AOG_SERVO_MAX_ACT)
    return fail(AOG_ERR_INVALID, "aog_servo_create: act_dim %d outside [1, %d]", cfg->act_dim, AOG_SERVO_MAX_ACT);
  if (cfg->max_latency < 0 || cfg->max_latency > AOG_SERVO_MAX_LATENCY)
    return fail(AOG_ERR_INVALID, "aog_servo_create: max_latency %d outside [0, %d]", cfg->max_latency, AOG_SERVO_MAX_LATENCY);
  // (the kernels index the ring with 32-bit env and actuator numbers)
  if ((long long)cfg->num_envs * cfg->act_dim * (cfg->max_latency + 2) > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "aog_servo_create: num_envs %d x act_dim %d x (max_latency + 2) exceeds 2^31 - 1 ring entries", cfg->num_envs, cfg->act_dim);
  HIP_TRY(hipSetDevice(device));
  aog_servo* g = new aog_servo;
  g->cfg = *cfg;
  const size_t n = cells(g);
  HostParams host(g);
  for (size_t b = 0; b < envs(g); ++b) {
    host.response[b] = 1.0;
    host.stroke[b] = HUGE_VAL;
  }
  hipError_t err = g->state.alloc(device, sizeof(double) * n + sizeof(unsigned long long) + sizeof(float) * n * depth(g));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&g->params), host.bytes.size());
  // the state starts as zeros; the fill runs on the null stream, which a caller's non-blocking stream does not wait for
  if (err == hipSuccess) err = hipMemset(g->state.ptr, 0, g->state.bytes);
  if (err == hipSuccess) err = hipMemcpy(g->params, host.bytes.data(), host.bytes.size(), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  if (err != hipSuccess) {
    release(g);
    return fail(AOG_ERR_HIP, "aog_servo_create: %s", hipGetErrorString(err));
  }
  *out = g;
  return AOG_OK;
}

void aog_servo_destroy(aog_servo* g) {
  if (!g) return;
  (void)hipSetDevice(g->state.device);
  release(g);
}

int aog_servo_set_params(aog_servo* g, const double* latency, const double* response, const double* stroke, const uint8_t* stuck,
                         const float* stuck_value) {
  REFUSE_NULL("aog_servo_set_params", {"servo", g}, {"latency_host", latency}, {"response_host", response}, {"stroke_host", stroke}, {"stuck_host", stuck},
              {"stuck_value_host", stuck_value});
  HostParams host(g);
  const int A = g->cfg.act_dim;
  for (size_t b = 0; b < envs(g); ++b) {
    const int env = (int)b;
    if (!(latency[b] >= 0.0 && latency[b] <= (double)g->cfg.max_latency))
      return fail(AOG_ERR_INVALID, "aog_servo_set_params: latency[%d] = %g outside [0, max_latency = %d]", env, latency[b], g->cfg.max_latency);
    if (!(response[b] > 0.0 && response[b] <= 1.0)) return fail(AOG_ERR_INVALID, "aog_servo_set_params: response[%d] = %g outside (0, 1]", env, response[b]);
    if (!(stroke[b] > 0.0)) return fail(AOG_ERR_INVALID, "aog_servo_set_params: stroke[%d] = %g must be > 0 (+inf: no limit)", env, stroke[b]);
    const double d = std::floor(latency[b]);
    host.delay[b] = (int32_t)d;
    host.frac[b] = latency[b] - d;
    host.response[b] = response[b];
    host.stroke[b] = stroke[b];
    for (int j = 0; j < A; ++j) {
      const float v = stuck_value[b * A + j];
      if (!std::isfinite(v)) return fail(AOG_ERR_INVALID, "aog_servo_set_params: stuck_value[%d][%d] = %g is not finite", env, j, (double)v);
      host.stuck_value[b * A + j] = v;
      host.stuck[b * A + j] = stuck[b * A + j] ? 1 : 0;
    }
  }
  HIP_TRY(hipSetDevice(g->state.device));
  HIP_TRY(hipMemcpy(g->params, host.bytes.data(), host.bytes.size(), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_servo_reset(aog_servo* g, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_servo_reset", {"servo", g});
  const aog::ServoArgs a = servo_args(g, nullptr, mask_dev, nullptr);
  LAUNCH_PLAIN(g->state.device, stream, aog::k_servo_reset, grid_of(g), dim3(256), a.y, a.ring, mask_dev, a.B, a.A, a.R);
  return AOG_OK;
}

int aog_servo_apply(aog_servo* g, const float* action_in_dev, const uint8_t* mask_dev, float* action_out_dev, void* stream) {
  REFUSE_NULL("aog_servo_apply", {"servo", g}, {"action_in_dev", action_in_dev}, {"action_out_dev", action_out_dev});
  LAUNCH_PLAIN(g->state.device, stream, aog::k_servo_apply, grid_of(g), dim3(256), servo_args(g, action_in_dev, mask_dev, action_out_dev));
  g->calls += 1;
  return AOG_OK;
}

int64_t aog_servo_state_bytes(const aog_servo* g) { return g ? (int64_t)g->state.bytes : 0; }

int aog_servo_get_state(aog_servo* g, void* blob_dev, void* stream) {
  REFUSE_NULL("aog_servo_get_state", {"servo", g}, {"blob_dev", blob_dev});
  return g->state.copy_out(blob_dev, stream);
}

int aog_servo_set_state(aog_servo* g, const void* blob_dev, void* stream) {
  REFUSE_NULL("aog_servo_set_state", {"servo", g}, {"blob_dev", blob_dev});
  if (int rc = g->state.copy_in(blob_dev, stream)) return rc;
  // the host's counter comes back from the blob: the one wait of this handle's calls
  unsigned long long calls = 0;
  HIP_TRY(hipMemcpyAsync(&calls, g->state.ptr + counter_offset(g), sizeof calls, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  g->calls = calls;
  return AOG_OK;
}

}  // extern "C"
