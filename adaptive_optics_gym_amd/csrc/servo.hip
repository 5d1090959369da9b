// K22: the mirror servo (aog_servo_*): loop latency, first-order mirror response, finite stroke and stuck actuators between the commanded
// action and the action the mirror receives.  Independent of any aog_env; whoever owns the handle steps the env with what it writes.
#include "standalone_handle.h"
#include "k_servo.h"
#include "../../include/aogym_servo.h"

using namespace aog_host;

struct aog_servo : StandaloneHandle<aog_servo_config> {   // state: y [B][A] float64, counter (uint64), ring [B][R][A] float32 (k_servo.h)
  char* params = nullptr;       // the block ServoParams carves
  unsigned long long calls = 0; // the counter, kept here: every aog_servo_apply hands n mod R and n + 1 to its launch
};

namespace {

size_t envs(const aog_servo* g) { return (size_t)g->cfg.num_envs; }
size_t cells(const aog_servo* g) { return envs(g) * g->cfg.act_dim; }
int depth(const aog_servo* g) { return g->cfg.max_latency + 2; }
size_t counter_offset(const aog_servo* g) { return sizeof(double) * cells(g); }

// The parameter block, on the host and on the device: frac | response | stroke ([B] float64 each) | stuck_value ([B][A] float32) |
// delay ([B] int32) | stuck ([B][A] uint8), carved from `base` for B envs and n = B A cells (base null: only `bytes` means anything)
struct ServoParams {
  double *frac, *response, *stroke;
  float* stuck_value;
  int32_t* delay;
  uint8_t* stuck;
  size_t bytes = 0;
  ServoParams(char* base, size_t B, size_t n) {
    auto take = [&](auto*& p, size_t count) {
      p = base ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + bytes) : nullptr;
      bytes += count * sizeof(*p);
    };
    take(frac, B), take(response, B), take(stroke, B), take(stuck_value, n), take(delay, B), take(stuck, n);
  }
};
size_t param_bytes(const aog_servo* g) { return ServoParams(nullptr, envs(g), cells(g)).bytes; }

// the block as it goes to the device, staged on the host
struct HostParams {
  std::vector<char> bytes;
  ServoParams at;
  explicit HostParams(const aog_servo* g) : bytes(param_bytes(g), 0), at(bytes.data(), envs(g), cells(g)) {}
};

aog::ServoArgs servo_args(const aog_servo* g, const float* in, const uint8_t* mask, float* out) {
  const ServoParams p(g->params, envs(g), cells(g));
  aog::ServoArgs a{};
  a.y = reinterpret_cast<double*>(g->state.ptr);
  a.counter = reinterpret_cast<unsigned long long*>(g->state.ptr + counter_offset(g));
  a.ring = reinterpret_cast<float*>(g->state.ptr + counter_offset(g) + sizeof(unsigned long long));
  a.frac = p.frac;
  a.response = p.response;
  a.stroke = p.stroke;
  a.stuck_value = p.stuck_value;
  a.delay = p.delay;
  a.stuck = p.stuck;
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

int servo_check(const aog_servo_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_servo_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_servo_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->act_dim < 1 || cfg->act_dim > AOG_SERVO_MAX_ACT)
    return fail(AOG_ERR_INVALID, "aog_servo_create: act_dim %d outside [1, %d]", cfg->act_dim, AOG_SERVO_MAX_ACT);
  if (cfg->max_latency < 0 || cfg->max_latency > AOG_SERVO_MAX_LATENCY)
    return fail(AOG_ERR_INVALID, "aog_servo_create: max_latency %d outside [0, %d]", cfg->max_latency, AOG_SERVO_MAX_LATENCY);
  // (the kernels index the ring with 32-bit env and actuator numbers)
  if ((long long)cfg->num_envs * cfg->act_dim * (cfg->max_latency + 2) > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "aog_servo_create: num_envs %d x act_dim %d x (max_latency + 2) exceeds 2^31 - 1 ring entries", cfg->num_envs, cfg->act_dim);
  return AOG_OK;
}

}  // namespace

extern "C" {

int64_t aog_servo_config_size(void) { return (int64_t)sizeof(aog_servo_config); }

int aog_servo_create(const aog_servo_config* cfg, int device, aog_servo** out) {
  // the state starts as zeros, the parameters as the identity until aog_servo_set_params
  return handle_create("aog_servo_create", cfg, device, out, servo_check, [](aog_servo* g) {
    const size_t n = cells(g);
    HostParams host(g);
    for (size_t b = 0; b < envs(g); ++b) {
      host.at.response[b] = 1.0;
      host.at.stroke[b] = HUGE_VAL;
    }
    if (hipError_t err = g->alloc_state(sizeof(double) * n + sizeof(unsigned long long) + sizeof(float) * n * depth(g), true)) return err;
    if (hipError_t err = g->own(&g->params, host.bytes.size(), false)) return err;
    return hipMemcpy(g->params, host.bytes.data(), host.bytes.size(), hipMemcpyHostToDevice);
  });
}

void aog_servo_destroy(aog_servo* g) { handle_destroy(g); }

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
    host.at.delay[b] = (int32_t)d;
    host.at.frac[b] = latency[b] - d;
    host.at.response[b] = response[b];
    host.at.stroke[b] = stroke[b];
    for (int j = 0; j < A; ++j) {
      const float v = stuck_value[b * A + j];
      if (!std::isfinite(v)) return fail(AOG_ERR_INVALID, "aog_servo_set_params: stuck_value[%d][%d] = %g is not finite", env, j, (double)v);
      host.at.stuck_value[b * A + j] = v;
      host.at.stuck[b * A + j] = stuck[b * A + j] ? 1 : 0;
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

int64_t aog_servo_state_bytes(const aog_servo* g) { return handle_state_bytes(g); }

int aog_servo_get_state(aog_servo* g, void* blob_dev, void* stream) { return handle_get_state("aog_servo_get_state", "servo", g, blob_dev, stream); }

int aog_servo_set_state(aog_servo* g, const void* blob_dev, void* stream) {
  if (int rc = handle_set_state("aog_servo_set_state", "servo", g, blob_dev, stream)) return rc;
  // the host's counter comes back from the blob: the one wait of this handle's calls
  unsigned long long calls = 0;
  HIP_TRY(hipMemcpyAsync(&calls, g->state.ptr + counter_offset(g), sizeof calls, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  g->calls = calls;
  return AOG_OK;
}

}  // extern "C"
