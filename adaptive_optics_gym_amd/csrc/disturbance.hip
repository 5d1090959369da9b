// K21: the modal disturbance's generator (aog_disturbance_*): a static offset plus an AR(2) vibration per (env, term).  Independent of any
// aog_env; what it writes is the coefficient array aog_install_layer_sum_disturbed (layers.hip) reads.
#include "standalone_handle.h"
#include "k_disturbance.h"
#include "../../include/aogym_disturbance.h"

using namespace aog_host;

struct aog_disturbance : StandaloneHandle<aog_disturbance_config> {   // state: x [B][K], x_prev [B][K], counter (k_disturbance.h)
  double* params = nullptr;   // [kRows][B][K], rows in Row's order
};

namespace {

// the rows of the parameter block, on the host and on the device: the six of aog_disturbance_set_params, then sqrt(1 - rho1 rho1)
enum Row { kA1, kA2, kB, kSigma, kRho1, kOffset, kRoot, kRows };
double* row(double* params, size_t n, int r) { return params + (size_t)r * n; }

size_t cells(const aog_disturbance* g) { return (size_t)g->cfg.num_envs * g->cfg.n_terms; }

int disturbance_check(const aog_disturbance_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_disturbance_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_disturbance_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->n_terms < 1 || cfg->n_terms > AOG_DISTURBANCE_MAX_TERMS)
    return fail(AOG_ERR_INVALID, "aog_disturbance_create: n_terms %d outside [1, %d]", cfg->n_terms, AOG_DISTURBANCE_MAX_TERMS);
  return AOG_OK;
}

aog::DisturbanceArgs dist_args(const aog_disturbance* g, int mode, const uint8_t* mask, double* coeff, double* noise) {
  const size_t n = cells(g);
  double* st = reinterpret_cast<double*>(g->state.ptr);
  aog::DisturbanceArgs a{};
  a.x = st;
  a.x_prev = st + n;
  a.counter = reinterpret_cast<const unsigned long long*>(st + 2 * n);
  a.a1 = row(g->params, n, kA1);
  a.a2 = row(g->params, n, kA2);
  a.b = row(g->params, n, kB);
  a.sigma = row(g->params, n, kSigma);
  a.rho1 = row(g->params, n, kRho1);
  a.offset = row(g->params, n, kOffset);
  a.root = row(g->params, n, kRoot);
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

}  // namespace

extern "C" {

int64_t aog_disturbance_config_size(void) { return (int64_t)sizeof(aog_disturbance_config); }

int aog_disturbance_create(const aog_disturbance_config* cfg, int device, aog_disturbance** out) {
  // state and parameters start as zeros
  return handle_create("aog_disturbance_create", cfg, device, out, disturbance_check, [](aog_disturbance* g) {
    if (hipError_t err = g->alloc_state(2 * sizeof(double) * cells(g) + sizeof(unsigned long long), true)) return err;
    return g->own(&g->params, kRows * sizeof(double) * cells(g), true);
  });
}

void aog_disturbance_destroy(aog_disturbance* g) { handle_destroy(g); }

int aog_disturbance_set_params(aog_disturbance* g, const double* a1, const double* a2, const double* b, const double* sigma, const double* rho1,
                               const double* offset) {
  REFUSE_NULL("aog_disturbance_set_params", {"gen", g}, {"a1_host", a1}, {"a2_host", a2}, {"b_host", b}, {"sigma_host", sigma}, {"rho1_host", rho1},
              {"offset_host", offset});
  const size_t n = cells(g);
  const double* rows[kRoot] = {a1, a2, b, sigma, rho1, offset};
  const char* names[kRoot] = {"a1", "a2", "b", "sigma", "rho1", "offset"};
  std::vector<double> host(kRows * n);
  for (int r = 0; r < kRoot; ++r)
    for (size_t i = 0; i < n; ++i) {
      const double v = rows[r][i];
      const int env = (int)(i / g->cfg.n_terms), k = (int)(i % g->cfg.n_terms);
      if (!std::isfinite(v)) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: %s[%d][%d] = %g is not finite", names[r], env, k, v);
      if (r == kSigma && v < 0.0) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: sigma[%d][%d] = %g must be >= 0", env, k, v);
      if (r == kRho1 && std::fabs(v) > 1.0) return fail(AOG_ERR_INVALID, "aog_disturbance_set_params: rho1[%d][%d] = %g outside [-1, 1]", env, k, v);
      row(host.data(), n, r)[i] = v;
    }
  for (size_t i = 0; i < n; ++i) {   // the stationary start's root, each operation rounded on its own
    volatile double square = rho1[i] * rho1[i];
    volatile double rest = 1.0 - square;
    row(host.data(), n, kRoot)[i] = std::sqrt(rest);
  }
  HIP_TRY(hipSetDevice(g->state.device));
  HIP_TRY(hipMemcpy(g->params, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_disturbance_reset(aog_disturbance* g, const uint8_t* mask_dev, double* noise_out, void* stream) {
  REFUSE_NULL("aog_disturbance_reset", {"gen", g});
  return run(g, aog::kDistReset, mask_dev, nullptr, noise_out, stream);
}

int aog_disturbance_advance(aog_disturbance* g, const uint8_t* mask_dev, double* coeff_out, double* noise_out, void* stream) {
  REFUSE_NULL("aog_disturbance_advance", {"gen", g}, {"coeff_out", coeff_out});
  return run(g, aog::kDistAdvance, mask_dev, coeff_out, noise_out, stream);
}

int aog_disturbance_coefficients(aog_disturbance* g, double* coeff_out, void* stream) {
  REFUSE_NULL("aog_disturbance_coefficients", {"gen", g}, {"coeff_out", coeff_out});
  return run(g, aog::kDistPeek, nullptr, coeff_out, nullptr, stream);
}

int64_t aog_disturbance_state_bytes(const aog_disturbance* g) { return handle_state_bytes(g); }

int aog_disturbance_get_state(aog_disturbance* g, void* blob_dev, void* stream) {
  return handle_get_state("aog_disturbance_get_state", "gen", g, blob_dev, stream);
}

int aog_disturbance_set_state(aog_disturbance* g, const void* blob_dev, void* stream) {
  return handle_set_state("aog_disturbance_set_state", "gen", g, blob_dev, stream);
}

}  // extern "C"
