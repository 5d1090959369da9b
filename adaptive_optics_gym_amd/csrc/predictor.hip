// K17: the predictive linear controller's per-env recursive-least-squares state (aog_predictor_*).  Independent of any aog_env.
#include "standalone_handle.h"
#include "k_predictor.h"

using namespace aog_host;

struct aog_predictor : StandaloneHandle<aog_predictor_config> {   // state: [batch] records (k_predictor.h)
  int n = 0;
  size_t rec_bytes = 0;
};

namespace {

// the checks of a configuration, before any device work
int predictor_check(const aog_predictor_config* c) {
  if (c->reserved0 != 0 || c->reserved1 != 0) return fail(AOG_ERR_INVALID, "aog_predictor_create: reserved fields must be 0");
  if (c->batch < 1 || c->act_dim < 1 || c->act_dim > aog::kPredMaxN || c->order < 1)
    return fail(AOG_ERR_INVALID, "aog_predictor_create: bad dimensions (batch %d, act_dim %d, order %d; act_dim <= %d)", c->batch, c->act_dim, c->order,
                aog::kPredMaxN);
  if (!(c->forgetting > 0.0 && c->forgetting <= 1.0)) return fail(AOG_ERR_INVALID, "aog_predictor_create: forgetting %g outside (0, 1]", c->forgetting);
  if (!std::isfinite(c->p0) || !(c->p0 > 0.0)) return fail(AOG_ERR_INVALID, "aog_predictor_create: p0 %g must be finite and > 0", c->p0);
  if (!std::isfinite(c->scale) || !(c->scale > 0.0)) return fail(AOG_ERR_INVALID, "aog_predictor_create: scale %g must be finite and > 0", c->scale);
  if ((int64_t)c->act_dim * c->order > aog::kPredMaxN)
    return fail(AOG_ERR_UNSUPPORTED, "aog_predictor_create: n = act_dim %d x order %d = %lld regressor entries; built for n <= %d", c->act_dim, c->order,
                (long long)c->act_dim * c->order, aog::kPredMaxN);
  return AOG_OK;
}

aog::PredictorArgs predictor_args(const aog_predictor* p, const uint8_t* mask) {
  aog::PredictorArgs a{};
  a.state = p->state.ptr;
  a.rec_bytes = p->rec_bytes;
  a.mask = mask;
  a.A = p->cfg.act_dim;
  a.order = p->cfg.order;
  a.n = p->n;
  a.lam = p->cfg.forgetting;
  a.scale = p->cfg.scale;
  a.p0 = p->cfg.p0;
  return a;
}

template <int NW, int RPW, int CB, int CBW, bool KEEP>
int launch_update(const aog_predictor* p, const aog::PredictorArgs& a, hipStream_t s) {
  const size_t lds = aog::predictor_lds_words(a.A, a.n, NW) * sizeof(double);   // <= 46 KB at n = A = 256
  return launch_with_lds(p->state.device, s, aog::k_predictor_update<NW, RPW, CB, CBW, KEEP>, dim3(p->cfg.batch), dim3(NW * 64), lds, a);
}

}  // namespace

extern "C" {

int aog_predictor_create(const aog_predictor_config* cfg, int device, aog_predictor** out) {
  return handle_create("aog_predictor_create", cfg, device, out, predictor_check, [](aog_predictor* p) {
    p->n = p->cfg.act_dim * p->cfg.order;
    p->rec_bytes = aog::predictor_record_words(p->cfg.act_dim, p->n) * sizeof(double);
    if (hipError_t err = p->alloc_state(p->rec_bytes * (size_t)p->cfg.batch, false)) return err;
    hipLaunchKernelGGL(aog::k_predictor_reset, dim3(p->cfg.batch), dim3(256), 0, nullptr, predictor_args(p, nullptr));
    return hipGetLastError();
  });
}

void aog_predictor_destroy(aog_predictor* p) { handle_destroy(p); }

int aog_predictor_reset(aog_predictor* p, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_predictor_reset", {"p", p});
  LAUNCH_PLAIN(p->state.device, stream, aog::k_predictor_reset, dim3(p->cfg.batch), dim3(256), predictor_args(p, mask_dev));
  return AOG_OK;
}

int aog_predictor_update(aog_predictor* p, const double* y_dev, const uint8_t* mask_dev, double* pred_dev, double* innov_dev, void* stream) {
  REFUSE_NULL("aog_predictor_update", {"p", p}, {"y_dev", y_dev}, {"pred_dev", pred_dev});
  HIP_TRY(hipSetDevice(p->state.device));
  aog::PredictorArgs a = predictor_args(p, mask_dev);
  a.y = y_dev;
  a.pred = pred_dev;
  a.innov = innov_dev;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the register forms hold the wave's rows of P and W (k_predictor.h); above kPredKeepN the two-read form
  if (p->n <= 64) return launch_update<4, 16, 1, 1, true>(p, a, s);
  if (p->n <= aog::kPredKeepN && a.A <= 64) return launch_update<8, 16, 2, 1, true>(p, a, s);
  if (p->n <= aog::kPredKeepN) return launch_update<8, 16, 2, 2, true>(p, a, s);
  return launch_update<8, 0, 4, 4, false>(p, a, s);
}

int64_t aog_predictor_state_bytes(const aog_predictor* p) { return handle_state_bytes(p); }

int aog_predictor_get_state(aog_predictor* p, void* blob_dev, void* stream) {
  return handle_get_state("aog_predictor_get_state", "p", p, blob_dev, stream);
}

int aog_predictor_set_state(aog_predictor* p, const void* blob_dev, void* stream) {
  return handle_set_state("aog_predictor_set_state", "p", p, blob_dev, stream);
}

}  // extern "C"
