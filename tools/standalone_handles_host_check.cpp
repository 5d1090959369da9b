// Host-side check of the stand-alone handles' paths that need no device, for a sanitizer build on a machine without a GPU:
//   - every config refusal of the six *_create calls and their null arguments,
//   - the null-argument refusal of every other entry point (the handle it gets is a block of zeros: nothing may look at it first),
//   - destroy and state_bytes of NULL,
//   - the carving of the servo's parameter block and the rows of the disturbance's, against offsets worked out by hand for B = 3, A = 5.
// It links the six units without the core unit and supplies the three functions they need of it.  The sanitizers go to the host side only
// (-Xarch_host, which also links their runtime); the device code is compiled as ever and never runs.  From the repository root:
//   cd tools && U=../adaptive_optics_gym_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined standalone_handles_host_check.cpp $U/predictor.hip $U/telemetry.hip $U/spgd.hip $U/link.hip \
//     -o standalone_handles_host_check && ./standalone_handles_host_check
#include "../adaptive_optics_gym_amd/csrc/servo.hip"
#include "../adaptive_optics_gym_amd/csrc/disturbance.hip"

#include <cstdarg>
#include <string>

static std::string g_error;
namespace aog_host {
int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}
int ensure_dynamic_lds(const void*, size_t, int) { return AOG_OK; }
}  // namespace aog_host

static int g_checks = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    ++g_checks;                                                             \
    if (!(cond)) {                                                          \
      std::printf("%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static bool says(const char* a, const char* b = "") { return g_error.find(a) != std::string::npos && g_error.find(b) != std::string::npos; }
static bool ends(const std::string& tail) { return g_error.size() >= tail.size() && g_error.compare(g_error.size() - tail.size(), tail.size(), tail) == 0; }

// cfg with one field changed must be refused with `code`, naming the entry point and the field, and leave *out null
template <typename H, typename Config, typename Field, typename Value>
static bool refused(int (*create)(const Config*, int, H**), const char* who, Config cfg, Field Config::*field, Value v, const char* word,
                    int code = AOG_ERR_INVALID) {
  cfg.*field = (Field)v;
  H* out = reinterpret_cast<H*>(0x5A);
  return create(&cfg, 0, &out) == code && says(who, word) && out == nullptr;
}

int main() {
  alignas(16) static char zeros[4096];
  void* some = zeros;
  double ascending[4] = {0.25, 0.5, 1.0, 2.0};

  // ---- create: null arguments, then every config refusal
  {
    const aog_predictor_config good{2, 8, 2, 0, 0, 0, 0.999, 1e3, 2e-7};
    aog_predictor* out = nullptr;
    EXPECT(aog_predictor_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_predictor_create: null argument cfg"));
    EXPECT(aog_predictor_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_create: null argument out"));
    const char* who = "aog_predictor_create";
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::batch, 0, "batch"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::act_dim, 0, "act_dim"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::act_dim, 257, "act_dim"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::order, 0, "order"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::reserved0, 1, "reserved"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::reserved1, 7, "reserved"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::forgetting, 0.0, "forgetting"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::forgetting, NAN, "forgetting"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::p0, HUGE_VAL, "p0"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::scale, -1.0, "scale"));
    EXPECT(refused(aog_predictor_create, who, good, &aog_predictor_config::order, 200, "order", AOG_ERR_UNSUPPORTED));
  }
  {
    const aog_telemetry_config good{2, 8, 64, 0};
    aog_telemetry* out = nullptr;
    EXPECT(aog_telemetry_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_telemetry_create: null argument cfg"));
    EXPECT(aog_telemetry_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_create: null argument out"));
    const char* who = "aog_telemetry_create";
    EXPECT(refused(aog_telemetry_create, who, good, &aog_telemetry_config::batch, 0, "batch"));
    EXPECT(refused(aog_telemetry_create, who, good, &aog_telemetry_config::act_dim, 129, "act_dim"));
    EXPECT(refused(aog_telemetry_create, who, good, &aog_telemetry_config::length, 32, "length"));
    EXPECT(refused(aog_telemetry_create, who, good, &aog_telemetry_config::length, 96, "length"));
    EXPECT(refused(aog_telemetry_create, who, good, &aog_telemetry_config::length, 2048, "length"));
  }
  {
    aog_spgd_config good{};
    good.abi_version = AOG_ABI_VERSION, good.num_envs = 2, good.act_dim = 4, good.seed = 1;
    aog_spgd* out = nullptr;
    EXPECT(aog_spgd_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_spgd_create: null argument cfg"));
    EXPECT(aog_spgd_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_create: null argument out"));
    const char* who = "aog_spgd_create";
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::abi_version, AOG_ABI_VERSION - 1, "abi_version"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::num_envs, 0, "num_envs"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::act_dim, 0, "act_dim"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::metric, 3, "metric"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::reserved0, 1, "reserved"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::clip, -1.0, "clip"));
    EXPECT(refused(aog_spgd_create, who, good, &aog_spgd_config::clip, NAN, "clip"));
  }
  {
    const aog_link_config good{AOG_ABI_VERSION, 2, 64, 0, 0};
    aog_link* out = nullptr;
    EXPECT(aog_link_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_link_create: null argument cfg"));
    EXPECT(aog_link_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_link_create: null argument out"));
    const char* who = "aog_link_create";
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::abi_version, AOG_ABI_VERSION - 1, "abi_version"));
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::num_envs, -3, "num_envs"));
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::length, 32, "length"));
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::length, 96, "length"));
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::length, 8192, "length"));
    EXPECT(refused(aog_link_create, who, good, &aog_link_config::reserved, 1, "reserved"));
  }
  {
    const aog_disturbance_config good{AOG_ABI_VERSION, 4, 2, 0, 1};
    aog_disturbance* out = nullptr;
    EXPECT(aog_disturbance_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_disturbance_create: null argument cfg"));
    EXPECT(aog_disturbance_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_create: null argument out"));
    const char* who = "aog_disturbance_create";
    EXPECT(refused(aog_disturbance_create, who, good, &aog_disturbance_config::abi_version, AOG_ABI_VERSION - 1, "abi_version"));
    EXPECT(refused(aog_disturbance_create, who, good, &aog_disturbance_config::num_envs, 0, "num_envs"));
    EXPECT(refused(aog_disturbance_create, who, good, &aog_disturbance_config::n_terms, 0, "n_terms"));
    EXPECT(refused(aog_disturbance_create, who, good, &aog_disturbance_config::n_terms, AOG_DISTURBANCE_MAX_TERMS + 1, "n_terms"));
  }
  {
    const aog_servo_config good{AOG_ABI_VERSION, 4, 2, 1};
    aog_servo* out = nullptr;
    EXPECT(aog_servo_create(nullptr, 0, &out) == AOG_ERR_INVALID && ends("aog_servo_create: null argument cfg"));
    EXPECT(aog_servo_create(&good, 0, nullptr) == AOG_ERR_INVALID && ends("aog_servo_create: null argument out"));
    const char* who = "aog_servo_create";
    EXPECT(refused(aog_servo_create, who, good, &aog_servo_config::abi_version, AOG_ABI_VERSION - 1, "abi_version"));
    EXPECT(refused(aog_servo_create, who, good, &aog_servo_config::num_envs, 0, "num_envs"));
    EXPECT(refused(aog_servo_create, who, good, &aog_servo_config::act_dim, AOG_SERVO_MAX_ACT + 1, "act_dim"));
    EXPECT(refused(aog_servo_create, who, good, &aog_servo_config::max_latency, -1, "max_latency"));
    EXPECT(refused(aog_servo_create, who, good, &aog_servo_config::max_latency, AOG_SERVO_MAX_LATENCY + 1, "max_latency"));
    aog_servo_config huge{AOG_ABI_VERSION, 1 << 30, 128, 4};
    EXPECT(aog_servo_create(&huge, 0, &out) == AOG_ERR_INVALID && says("aog_servo_create", "num_envs") && !out);
  }

  // ---- destroy and state_bytes of NULL
  aog_predictor_destroy(nullptr), aog_telemetry_destroy(nullptr), aog_spgd_destroy(nullptr), aog_link_destroy(nullptr);
  aog_disturbance_destroy(nullptr), aog_servo_destroy(nullptr);
  EXPECT(aog_predictor_state_bytes(nullptr) == 0 && aog_telemetry_state_bytes(nullptr) == 0 && aog_spgd_state_bytes(nullptr) == 0);
  EXPECT(aog_link_state_bytes(nullptr) == 0 && aog_disturbance_state_bytes(nullptr) == 0 && aog_servo_state_bytes(nullptr) == 0);

  // ---- the other entry points: a null handle, then each required pointer in turn beside a handle of zeros
  auto P = (aog_predictor*)some;
  EXPECT(aog_predictor_reset(nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_reset: null argument p"));
  EXPECT(aog_predictor_update(nullptr, (double*)some, nullptr, (double*)some, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_update: null argument p"));
  EXPECT(aog_predictor_update(P, nullptr, nullptr, (double*)some, nullptr, nullptr) == AOG_ERR_INVALID && ends("null argument y_dev"));
  EXPECT(aog_predictor_update(P, (double*)some, nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("null argument pred_dev"));
  EXPECT(aog_predictor_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_get_state: null argument p"));
  EXPECT(aog_predictor_get_state(P, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_get_state: null argument blob_dev"));
  EXPECT(aog_predictor_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_set_state: null argument p"));
  EXPECT(aog_predictor_set_state(P, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_predictor_set_state: null argument blob_dev"));

  auto T = (aog_telemetry*)some;
  EXPECT(aog_telemetry_reset(nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_reset: null argument t"));
  EXPECT(aog_telemetry_push(nullptr, (double*)some, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_push: null argument t"));
  EXPECT(aog_telemetry_push(T, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_push: null argument y_dev"));
  EXPECT(aog_telemetry_psd(nullptr, 32, (double*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_psd: null argument t"));
  EXPECT(aog_telemetry_psd(T, 32, nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_psd: null argument psd_dev"));
  EXPECT(aog_telemetry_gains(nullptr, 32, 1, ascending, 4, (double*)some, (double*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_gains: null argument t"));
  EXPECT(aog_telemetry_gains(T, 32, 1, nullptr, 4, (double*)some, (double*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("null argument grid_host"));
  EXPECT(aog_telemetry_gains(T, 32, 1, ascending, 4, nullptr, (double*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("null argument gain_dev"));
  EXPECT(aog_telemetry_gains(T, 32, 1, ascending, 4, (double*)some, nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("null argument cost_dev"));
  EXPECT(aog_telemetry_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_get_state: null argument t"));
  EXPECT(aog_telemetry_get_state(T, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_get_state: null argument blob_dev"));
  EXPECT(aog_telemetry_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_set_state: null argument t"));
  EXPECT(aog_telemetry_set_state(T, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_telemetry_set_state: null argument blob_dev"));

  auto S = (aog_spgd*)some;
  EXPECT(aog_spgd_set_params(nullptr, ascending, ascending) == AOG_ERR_INVALID && ends("aog_spgd_set_params: null argument spgd"));
  EXPECT(aog_spgd_set_params(S, nullptr, ascending) == AOG_ERR_INVALID && ends("aog_spgd_set_params: null argument gain_host"));
  EXPECT(aog_spgd_set_params(S, ascending, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_set_params: null argument amplitude_host"));
  EXPECT(aog_spgd_reset(nullptr, nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_reset: null argument spgd"));
  EXPECT(aog_spgd_update(nullptr, (float*)some, nullptr, (float*)some, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_update: null argument spgd"));
  EXPECT(aog_spgd_update(S, nullptr, nullptr, (float*)some, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_update: null argument metric_dev"));
  EXPECT(aog_spgd_update(S, (float*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_update: null argument action_out"));
  EXPECT(aog_spgd_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_get_state: null argument spgd"));
  EXPECT(aog_spgd_get_state(S, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_get_state: null argument blob_dev"));
  EXPECT(aog_spgd_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_set_state: null argument spgd"));
  EXPECT(aog_spgd_set_state(S, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_spgd_set_state: null argument blob_dev"));

  auto L = (aog_link*)some;
  EXPECT(aog_link_reset(nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_link_reset: null argument link"));
  EXPECT(aog_link_push(nullptr, (float*)some, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_link_push: null argument link"));
  EXPECT(aog_link_push(L, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_link_push: null argument power_dev"));
  {
    // the required outputs in the order of the parameter list, then the arrays a count above 0 asks for
    void* req[8] = {L, some, some, some, some, some, some, some};   // link, samples, mean, mean_square, minimum, maximum, reference, hist
    const char* names[8] = {"link", "samples_dev", "mean_dev", "mean_square_dev", "minimum_dev", "maximum_dev", "reference_dev", "hist_dev"};
    auto stats = [&](void** r, const double* e, int ne, const double* h, int nh, const double* q, int nq, void* below, void* fades, void* longest, void* ber) {
      return aog_link_statistics((aog_link*)r[0], AOG_LINK_REF_MEAN, 0.0, e, ne, h, nh, q, nq, (int32_t*)r[1], (double*)r[2], (double*)r[3], (float*)r[4],
                                 (float*)r[5], (double*)r[6], (int32_t*)below, (int32_t*)fades, (int32_t*)longest, (int32_t*)r[7], (double*)ber, nullptr,
                                 nullptr);
    };
    for (int i = 0; i < 8; ++i) {
      void* r[8];
      std::copy(req, req + 8, r);
      r[i] = nullptr;
      EXPECT(stats(r, ascending, 4, ascending, 4, ascending, 4, some, some, some, some) == AOG_ERR_INVALID &&
             ends(std::string("aog_link_statistics: null argument ") + names[i]));
    }
    EXPECT(stats(req, nullptr, 4, ascending, 4, ascending, 4, some, some, some, some) == AOG_ERR_INVALID && ends("aog_link_statistics: null argument edges_rel"));
    EXPECT(stats(req, ascending, 4, nullptr, 4, ascending, 4, some, some, some, some) == AOG_ERR_INVALID && ends("null argument hist_edges_rel"));
    EXPECT(stats(req, ascending, 4, ascending, 4, nullptr, 4, some, some, some, some) == AOG_ERR_INVALID && ends("null argument q"));
    EXPECT(stats(req, ascending, 4, ascending, 4, ascending, 4, nullptr, some, some, some) == AOG_ERR_INVALID && ends("null argument below_dev"));
    EXPECT(stats(req, ascending, 4, ascending, 4, ascending, 4, some, nullptr, some, some) == AOG_ERR_INVALID && ends("null argument fades_dev"));
    EXPECT(stats(req, ascending, 4, ascending, 4, ascending, 4, some, some, nullptr, some) == AOG_ERR_INVALID && ends("null argument longest_dev"));
    EXPECT(stats(req, ascending, 4, ascending, 4, ascending, 4, some, some, some, nullptr) == AOG_ERR_INVALID && ends("null argument ber_dev"));
    EXPECT(stats(req, ascending, 17, ascending, 4, ascending, 4, some, some, some, some) == AOG_ERR_INVALID && says("edges_rel", "outside"));
  }
  EXPECT(aog_link_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_link_get_state: null argument link"));
  EXPECT(aog_link_get_state(L, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_link_get_state: null argument blob_dev"));
  EXPECT(aog_link_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_link_set_state: null argument link"));
  EXPECT(aog_link_set_state(L, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_link_set_state: null argument blob_dev"));

  auto D = (aog_disturbance*)some;
  {
    const char* names[7] = {"gen", "a1_host", "a2_host", "b_host", "sigma_host", "rho1_host", "offset_host"};
    for (int i = 0; i < 7; ++i) {
      const void* a[7] = {D, ascending, ascending, ascending, ascending, ascending, ascending};
      a[i] = nullptr;
      EXPECT(aog_disturbance_set_params((aog_disturbance*)a[0], (const double*)a[1], (const double*)a[2], (const double*)a[3], (const double*)a[4],
                                        (const double*)a[5], (const double*)a[6]) == AOG_ERR_INVALID &&
             ends(std::string("aog_disturbance_set_params: null argument ") + names[i]));
    }
  }
  EXPECT(aog_disturbance_reset(nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_reset: null argument gen"));
  EXPECT(aog_disturbance_advance(nullptr, nullptr, (double*)some, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_advance: null argument gen"));
  EXPECT(aog_disturbance_advance(D, nullptr, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_advance: null argument coeff_out"));
  EXPECT(aog_disturbance_coefficients(nullptr, (double*)some, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_coefficients: null argument gen"));
  EXPECT(aog_disturbance_coefficients(D, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_coefficients: null argument coeff_out"));
  EXPECT(aog_disturbance_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_get_state: null argument gen"));
  EXPECT(aog_disturbance_get_state(D, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_get_state: null argument blob_dev"));
  EXPECT(aog_disturbance_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_set_state: null argument gen"));
  EXPECT(aog_disturbance_set_state(D, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_disturbance_set_state: null argument blob_dev"));

  auto V = (aog_servo*)some;
  {
    const char* names[6] = {"servo", "latency_host", "response_host", "stroke_host", "stuck_host", "stuck_value_host"};
    for (int i = 0; i < 6; ++i) {
      const void* a[6] = {V, ascending, ascending, ascending, some, some};
      a[i] = nullptr;
      EXPECT(aog_servo_set_params((aog_servo*)a[0], (const double*)a[1], (const double*)a[2], (const double*)a[3], (const uint8_t*)a[4], (const float*)a[5]) ==
                 AOG_ERR_INVALID &&
             ends(std::string("aog_servo_set_params: null argument ") + names[i]));
    }
  }
  EXPECT(aog_servo_reset(nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_servo_reset: null argument servo"));
  EXPECT(aog_servo_apply(nullptr, (float*)some, nullptr, (float*)some, nullptr) == AOG_ERR_INVALID && ends("aog_servo_apply: null argument servo"));
  EXPECT(aog_servo_apply(V, nullptr, nullptr, (float*)some, nullptr) == AOG_ERR_INVALID && ends("aog_servo_apply: null argument action_in_dev"));
  EXPECT(aog_servo_apply(V, (float*)some, nullptr, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_servo_apply: null argument action_out_dev"));
  EXPECT(aog_servo_get_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_servo_get_state: null argument servo"));
  EXPECT(aog_servo_get_state(V, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_servo_get_state: null argument blob_dev"));
  EXPECT(aog_servo_set_state(nullptr, some, nullptr) == AOG_ERR_INVALID && ends("aog_servo_set_state: null argument servo"));
  EXPECT(aog_servo_set_state(V, nullptr, nullptr) == AOG_ERR_INVALID && ends("aog_servo_set_state: null argument blob_dev"));

  // ---- the servo's block at B = 3, A = 5 (n = 15): frac 0, response 24, stroke 48, stuck_value 72 (+ 15 x 4), delay 132 (+ 3 x 4), stuck 144, 159 bytes
  {
    const size_t B = 3, n = 15;
    EXPECT(ServoParams(nullptr, B, n).bytes == 159);
    aog_servo g;
    g.cfg = aog_servo_config{AOG_ABI_VERSION, 3, 5, 1};
    EXPECT(param_bytes(&g) == 159);
    HostParams host(&g);
    char* base = host.bytes.data();
    EXPECT(host.bytes.size() == 159 && host.at.bytes == 159);
    EXPECT((char*)host.at.frac == base && (char*)host.at.response == base + 24 && (char*)host.at.stroke == base + 48);
    EXPECT((char*)host.at.stuck_value == base + 72 && (char*)host.at.delay == base + 132 && (char*)host.at.stuck == base + 144);
    for (size_t b = 0; b < B; ++b) host.at.frac[b] = host.at.response[b] = host.at.stroke[b] = 1.0, host.at.delay[b] = 1;   // every byte of the block is the block's
    for (size_t i = 0; i < n; ++i) host.at.stuck_value[i] = 1.f, host.at.stuck[i] = 1;
    // what the kernel's arguments read of a device block is the same carving
    g.params = base;
    g.state.ptr = zeros;   // (the records' pointers are formed too)
    const aog::ServoArgs a = servo_args(&g, nullptr, nullptr, nullptr);
    EXPECT(a.frac == host.at.frac && a.response == host.at.response && a.stroke == host.at.stroke && a.stuck_value == host.at.stuck_value);
    EXPECT((const void*)a.delay == host.at.delay && a.stuck == host.at.stuck && a.B == 3 && a.A == 5 && a.R == 3);
    g.params = nullptr;
  }
  // ---- the disturbance's rows at B = 3, K = 5 (n = 15): row r starts at double 15 r; seven rows
  {
    std::vector<double> host(kRows * 15);
    EXPECT(kRows == 7 && kRoot == 6);
    for (int r = 0; r < kRows; ++r) {
      EXPECT(row(host.data(), 15, r) == host.data() + 15 * r);
      row(host.data(), 15, r)[14] = 1.0;
    }
    aog_disturbance g;
    g.cfg = aog_disturbance_config{AOG_ABI_VERSION, 3, 5, 0, 1};
    g.params = host.data();
    g.state.ptr = zeros;
    const aog::DisturbanceArgs a = dist_args(&g, aog::kDistPeek, nullptr, nullptr, nullptr);
    EXPECT(a.a1 == host.data() && a.a2 == host.data() + 15 && a.b == host.data() + 30 && a.sigma == host.data() + 45);
    EXPECT(a.rho1 == host.data() + 60 && a.offset == host.data() + 75 && a.root == host.data() + 90);
  }
  std::printf("standalone handles host check: %d checks passed\n", g_checks);
  return 0;
}
