// K21: the modal disturbance's generator (aog_disturbance_*): a static offset plus an AR(2) vibration per (env, term).  Independent of any
// aog_env; what it writes is the coefficient array aog_install_layer_sum_disturbed (layers.hip) reads.
#include "host_common.h"
#include "k_disturbance.h"
#include "../../include/aogym_disturbance.h"

using namespace aog_host;

struct aog_disturbance {
  aog_disturbance_config cfg{};
  RecordStore state;          // x [B][K], x_prev [B][K], counter (k_disturbance.h)
  double* params = nullptr;   // [7][B][K]: a1, a2, b, sigma, rho1, offset, sqrt(1 - rho1 rho1)
};

namespace {

size_t cells(const aog_disturbance* g) { return (size_t)g->cfg.num_envs * g->cfg.n_terms; }

aog::DisturbanceArgs dist_args(const aog_disturbance* g, int mode, const uint8_t* mask, double* coeff, double* noise) {
  const size_t n = cells(g);
  double* st = reinterpret_cast<double*>(g->state.ptr);
  aog::DisturbanceArgs a{};
  a.x = st;
  a.x_prev = st + n;
  a.counter = reinterpret_cast<const unsigned long long*>(st + 2 * n);
  a.a1 = g->params;
  a.a2 = g->params + n;
  a.b = g->params + 2 * n;
  a.sigma = g->params + 3 * n;
  a.rho1 = g->params + 4 * n;
  a.offset = g->params + 5 * n;
  a.root = g->params + 6 * n;
  a.mask = mask;
  a.coeff = coeff;
  a.noise = noise;
  a.B = g->cfg.num_envs;
  a.K = g->cfg.n_terms;
  a.env_base = g->cfg.env_id_base;
  a.mode = mode;
  a.seed = g->cfg.seed;
  return a;
}

// one call's kernel and, for the calls that draw, the counter's tick behind it
int run(aog_disturbance* g, int mode, const uint8_t* mask, double* coeff, double* noise, void* stream) {
  LAUNCH_PLAIN(g->state.device, stream, aog::k_disturbance, dim3((unsigned)((cells(g) + 255) / 256)), dim3(256), dist_args(g, mode, mask, coeff, noise));
  if (mode != aog::kDistPeek)
    LAUNCH_PLAIN(g->state.device, stream, aog::k_disturbance_tick, dim3(1), dim3(1),
                 reinterpret_cast<unsigned long long*>(g->state.ptr + 2 * sizeof(double) * cells(g)));
  return AOG_OK;
}

void release(aog_disturbance* g) {
  g->state.release();
  if (g->params) (void)hipFree(g->params);
  delete g;
}

}  // namespace

extern "C" {

int64_t aog_disturbance_config_size(void) { return (int64_t)sizeof(aog_disturbance_config); }

int aog_disturbance_create(const aog_disturbance_config* cfg, int device, aog_disturbance** out) {
  if (!cfg || !out) return fail(AOG_ERR_INVALID, "aog_disturbance_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_disturbance_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_disturbance_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->n_terms < 1 || cfg->n_terms > AOG_DISTURBANCE_MAX_TERMS)
    return fail(AOG_ERR_INVALID, "aog_disturbance_create: n_terms %d outside [1, %d]", cfg->n_terms, AOG_DISTURBANCE_MAX_TERMS);
  HIP_TRY(hipSetDevice(device));
  aog_disturbance* g = new aog_disturbance;
  g->cfg = *cfg;
  const size_t n = cells(g);
  hipError_t err = g->state.alloc(device, 2 * sizeof(double) * n + sizeof(unsigned long long));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&g->params), 7 * sizeof(double) * n);
  // state and parameters start as zeros; the fills run on the null stream, which a caller's non-blocking stream does not wait for
  if (err == hipSuccess) err = hipMemset(g->state.ptr, 0, g->state.bytes);
  if (err == hipSuccess) err = hipMemset(g->params, 0, 7 * sizeof(double) * n);
  if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  if (err != hipSuccess) {
    release(g);
    return fail(AOG_ERR_HIP, "aog_disturbance_create: %s", hipGetErrorString(err));
  }
  *out = g;
  return AOG_OK;
}

void aog_disturbance_destroy(aog_disturbance* g) {
  if (!g) return;
  (void)hipSetDevice(g->state.device);
  release(g);
}

int aog_disturbance_set_params(aog_disturbance* g, const double* a1, const double* a2, const double* b, const double* sigma, const double* rho1,
                               const double* offset) {
  if (!g || !a1 || !a2 || !b || !sigma || !rho1 || !offset) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: null argument");
  const size_t n = cells(g);
  const double* rows[6] = {a1, a2, b, sigma, rho1, offset};
  const char* names[6] = {"a1", "a2", "b", "sigma", "rho1", "offset"};
  std::vector<double> host(7 * n);
  for (int r = 0; r < 6; ++r)
    for (size_t i = 0; i < n; ++i) {
      const double v = rows[r][i];
      const int env = (int)(i / g->cfg.n_terms), k = (int)(i % g->cfg.n_terms);
      if (!std::isfinite(v)) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: %s[%d][%d] = %g is not finite", names[r], env, k, v);
      if (r == 3 && v < 0.0) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: sigma[%d][%d] = %g must be >= 0", env, k, v);
      if (r == 4 && std::fabs(v) > 1.0) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: rho1[%d][%d] = %g outside [-1, 1]", env, k, v);
      host[r * n + i] = v;
    }
  for (size_t i = 0; i < n; ++i) {   // the stationary start's root, each operation rounded on its own
    volatile double square = rho1[i] * rho1[i];
    volatile double rest = 1.0 - square;
    host[6 * n + i] = std::sqrt(rest);
  }
  HIP_TRY(hipSetDevice(g->state.device));
  HIP_TRY(hipMemcpy(g->params, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_disturbance_reset(aog_disturbance* g, const uint8_t* mask_dev, double* noise_out, void* stream) {
  if (!g) return fail(AOG_ERR_INVALID, "aog_disturbance_reset: null argument");
  return run(g, aog::kDistReset, mask_dev, nullptr, noise_out, stream);
}

int aog_disturbance_advance(aog_disturbance* g, const uint8_t* mask_dev, double* coeff_out, double* noise_out, void* stream) {
  if (!g || !coeff_out) return fail(AOG_ERR_INVALID, "aog_disturbance_advance: null argument");
  return run(g, aog::kDistAdvance, mask_dev, coeff_out, noise_out, stream);
}

int aog_disturbance_coefficients(aog_disturbance* g, double* coeff_out, void* stream) {
  if (!g || !coeff_out) return fail(AOG_ERR_INVALID, "aog_disturbance_coefficients: null argument");
  return run(g, aog::kDistPeek, nullptr, coeff_out, nullptr, stream);
}

int64_t aog_disturbance_state_bytes(const aog_disturbance* g) { return g ? (int64_t)g->state.bytes : 0; }

int aog_disturbance_get_state(aog_disturbance* g, void* blob_dev, void* stream) {
  if (!g || !blob_dev) return fail(AOG_ERR_INVALID, "aog_disturbance_get_state: null argument");
  return g->state.copy_out(blob_dev, stream);
}

int aog_disturbance_set_state(aog_disturbance* g, const void* blob_dev, void* stream) {
  if (!g || !blob_dev) return fail(AOG_ERR_INVALID, "aog_disturbance_set_state: null argument");
  return g->state.copy_in(blob_dev, stream);
}

}  // extern "C"
