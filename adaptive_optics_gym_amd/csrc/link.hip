// K20: link telemetry (aog_link_*): per-env rings of the fibre-coupled power and, over what they hold, fade statistics, the power
// histogram and the mean bit-error rate.  Independent of any aog_env.
#include "standalone_handle.h"
#include "k_link.h"

using namespace aog_host;

static_assert(aog::kLinkMaxK == AOG_LINK_MAX_EDGES && aog::kLinkMaxE == AOG_LINK_MAX_HIST && aog::kLinkMaxQ == AOG_LINK_MAX_Q, "link limits");

struct aog_link : StandaloneHandle<aog_link_config> {};   // state: [num_envs] records (k_link.h)

namespace {

int link_check(const aog_link_config* c) {
  if (c->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "aog_link_create: abi_version %d, the library is %d", c->abi_version, AOG_ABI_VERSION);
  if (c->reserved != 0) return fail(AOG_ERR_INVALID, "aog_link_create: reserved must be 0 (got %d)", c->reserved);
  if (c->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_link_create: num_envs %d must be >= 1", c->num_envs);
  if (c->length < aog::kLinkMinT || c->length > aog::kLinkMaxT || (c->length & (c->length - 1)) != 0)
    return fail(AOG_ERR_INVALID, "aog_link_create: length %d must be a power of two in [%d, %d]", c->length, aog::kLinkMinT, aog::kLinkMaxT);
  return AOG_OK;
}

aog::LinkArgs link_args(const aog_link* t, const uint8_t* mask) {
  aog::LinkArgs a{};
  a.state = t->state.ptr;
  a.rec_bytes = aog::link_record_bytes(t->cfg.length);
  a.mask = mask;
  a.B = t->cfg.num_envs;
  a.T = t->cfg.length;
  return a;
}

// `count` positive, finite, strictly ascending factors from src into dst
int copy_factors(const char* field, const double* src, int count, int limit, bool ascending, double* dst) {
  if (count < 0 || count > limit) return fail(AOG_ERR_INVALID, "aog_link_statistics: %d %s outside [0, %d]", count, field, limit);
  if (count > 0) REFUSE_NULL("aog_link_statistics", {field, src});
  for (int i = 0; i < count; ++i) {
    if (!std::isfinite(src[i]) || src[i] <= 0.0) return fail(AOG_ERR_INVALID, "aog_link_statistics: %s[%d] = %g must be positive and finite", field, i, src[i]);
    if (ascending && i && !(src[i] > src[i - 1]))
      return fail(AOG_ERR_INVALID, "aog_link_statistics: %s must ascend (%s[%d] = %g after %g)", field, field, i, src[i], src[i - 1]);
    dst[i] = src[i];
  }
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_link_create(const aog_link_config* cfg, int device, aog_link** out) {
  return handle_create("aog_link_create", cfg, device, out, link_check, [](aog_link* t) {
    if (hipError_t err = t->alloc_state(aog::link_record_bytes(t->cfg.length) * (size_t)t->cfg.num_envs, false)) return err;
    hipLaunchKernelGGL(aog::k_link_reset, dim3(t->cfg.num_envs), dim3(256), 0, nullptr, link_args(t, nullptr));
    return hipGetLastError();
  });
}

void aog_link_destroy(aog_link* t) { handle_destroy(t); }

int aog_link_reset(aog_link* t, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_link_reset", {"link", t});
  LAUNCH_PLAIN(t->state.device, stream, aog::k_link_reset, dim3(t->cfg.num_envs), dim3(256), link_args(t, mask_dev));
  return AOG_OK;
}

int aog_link_push(aog_link* t, const float* power_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_link_push", {"link", t}, {"power_dev", power_dev});
  aog::LinkArgs a = link_args(t, mask_dev);
  a.power = power_dev;
  LAUNCH_PLAIN(t->state.device, stream, aog::k_link_push, dim3((t->cfg.num_envs + 255) / 256), dim3(256), a);
  return AOG_OK;
}

int aog_link_statistics(aog_link* t, int reference_mode, double reference, const double* edges_rel, int n_edges, const double* hist_edges_rel,
                        int n_hist, const double* q, int n_q, int32_t* samples_dev, double* mean_dev, double* mean_square_dev, float* minimum_dev,
                        float* maximum_dev, double* reference_dev, int32_t* below_dev, int32_t* fades_dev, int32_t* longest_dev, int32_t* hist_dev,
                        double* ber_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_link_statistics", {"link", t}, {"samples_dev", samples_dev}, {"mean_dev", mean_dev}, {"mean_square_dev", mean_square_dev},
              {"minimum_dev", minimum_dev}, {"maximum_dev", maximum_dev}, {"reference_dev", reference_dev}, {"hist_dev", hist_dev});
  if (reference_mode != AOG_LINK_REF_ABSOLUTE && reference_mode != AOG_LINK_REF_MEAN)
    return fail(AOG_ERR_INVALID, "aog_link_statistics: reference_mode %d (0 = absolute, 1 = mean)", reference_mode);
  if (reference_mode == AOG_LINK_REF_ABSOLUTE && (!std::isfinite(reference) || reference <= 0.0))
    return fail(AOG_ERR_INVALID, "aog_link_statistics: reference %g must be positive and finite", reference);
  aog::LinkStatArgs a{};
  if (int rc = copy_factors("edges_rel", edges_rel, n_edges, aog::kLinkMaxK, true, a.f)) return rc;
  if (int rc = copy_factors("hist_edges_rel", hist_edges_rel, n_hist, aog::kLinkMaxE, true, a.g)) return rc;
  if (int rc = copy_factors("q", q, n_q, aog::kLinkMaxQ, false, a.q)) return rc;
  // (below, fades and longest go with edges_rel, ber with q)
  if (n_edges > 0) REFUSE_NULL("aog_link_statistics", {"below_dev", below_dev}, {"fades_dev", fades_dev}, {"longest_dev", longest_dev});
  if (n_q > 0) REFUSE_NULL("aog_link_statistics", {"ber_dev", ber_dev});
  a.h = link_args(t, mask_dev);
  a.mean_reference = reference_mode == AOG_LINK_REF_MEAN;
  a.reference = reference;
  a.K = n_edges;
  a.E = n_hist;
  a.Q = n_q;
  a.samples = samples_dev;
  a.mean = mean_dev;
  a.mean_square = mean_square_dev;
  a.minimum = minimum_dev;
  a.maximum = maximum_dev;
  a.level = reference_dev;
  a.below = below_dev;
  a.fades = fades_dev;
  a.longest = longest_dev;
  a.hist = hist_dev;
  a.ber = ber_dev;
  HIP_TRY(hipSetDevice(t->state.device));
  const int B = t->cfg.num_envs;
  return launch_with_lds(t->state.device, static_cast<hipStream_t>(stream), aog::k_link_statistics, dim3((B + aog::kLinkEnvs - 1) / aog::kLinkEnvs),
                         dim3(64 * aog::kLinkEnvs), aog::kLinkEnvs * aog::link_wave_lds_bytes(t->cfg.length), a);
}

int64_t aog_link_state_bytes(const aog_link* t) { return handle_state_bytes(t); }

int aog_link_get_state(aog_link* t, void* blob_dev, void* stream) { return handle_get_state("aog_link_get_state", "link", t, blob_dev, stream); }

int aog_link_set_state(aog_link* t, const void* blob_dev, void* stream) { return handle_set_state("aog_link_set_state", "link", t, blob_dev, stream); }

}  // extern "C"
