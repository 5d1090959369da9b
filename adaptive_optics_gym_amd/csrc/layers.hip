// Layered atmosphere (several frozen-flow layers per env): the atmosphere-only step of a layer handle and the installation of the layers'
// sum in a quasi-static front handle, plain, with a modal disturbance added inside the sum, or read along a sightline (layers larger than
// the front, displaced by a fraction of a pixel; altitude mirrors' surfaces as further sources), or from a source at finite range (the
// footprint on every source shrunk by a magnification).  A handle that never comes here launches nothing of this file.
#include "host_common.h"
#include "conjugate_host.h"
#include "k_layers.h"
#include "k_cone.h"
#include "../../include/aogym_disturbance.h"
#include "../../include/aogym_sightline.h"
#include "../../include/aogym_cone.h"

using namespace aog_host;

static_assert(aog::kMaxTerms == AOG_DISTURBANCE_MAX_TERMS, "the disturbance's term limit");

namespace {

// which of the four installations: what reads the layers and what is added inside the sum
enum class LayerForm {
  plain,       // aog_install_layer_sum: layers in the pupil plane, no terms
  disturbed,   // aog_install_layer_sum_disturbed: layers in the pupil plane, the uploaded basis's terms
  sightline,   // aog_install_layer_sum_sightline, aog_install_layer_sum_conjugate: sources of N_l >= N read at `shift_host`, terms when n_terms > 0
  cone,        // aog_install_layer_sum_cone: the sightline form with (sx, sy, m) per source and env in `shift_host`
};

// one source of a sightline installation as the margin check names it: layer l, or mirror j behind the layers
struct SightSource {
  const char* kind;
  int index, n;   // N_l
};

// The two launches of one installation.  Pass 1 reads every master once; pass 2 reads them again (8 n_ap bytes per env and layer, mostly
// from L2 / Infinity Cache; along a sightline four samples per pixel and layer, neighbours of a line already requested); ModalTerms add
// the K basis rows (8 K n_ap bytes, shared by every env: L2) to each pass.
template <int L, class Layers, class Terms>
void launch_passes(const Layers& layers, const Terms& terms, const aog_env* dst, hipStream_t s) {
  const aog::LayerSum<Layers, Terms> sum{layers, terms};
  const int N = dst->cfg.n_pupil;
  hipLaunchKernelGGL((aog::k_layer_mean<L, Layers, Terms>), dim3(dst->B), dim3(256), 0, s, sum, dst->ap_index, dst->layer_mean, N, dst->n_ap);
  if (dst->cfg.precision == AOG_PRECISION_FAST) {
    const dim3 tiles(((dst->n_ptiles + 1) / 2 + aog::kLayerIters - 1) / aog::kLayerIters, dst->n_etiles);
    hipLaunchKernelGGL((aog::k_layer_sum_tiles<L, Layers, Terms>), tiles, dim3(256), 0, s, sum, dst->ap_index, dst->layer_mean, dst->psi_tile, dst->B, N, dst->n_ap,
                       dst->n_ptiles, rev_per_metre(dst));
  } else {
    hipLaunchKernelGGL((aog::k_layer_sum_f64<L, Layers, Terms>), dim3(dst->B), dim3(256), 0, s, sum, dst->ap_index, dst->layer_mean, dst->psi64, N, dst->n_ap);
  }
}
// ... for the run-time layer count (1 .. kMaxLayers)
template <class Layers, class Terms>
void launch_passes(int n_layers, const Layers& layers, const Terms& terms, const aog_env* dst, hipStream_t s) {
  switch (n_layers) {
    case 1: return launch_passes<1>(layers, terms, dst, s);
    case 2: return launch_passes<2>(layers, terms, dst, s);
    case 3: return launch_passes<3>(layers, terms, dst, s);
    case 4: return launch_passes<4>(layers, terms, dst, s);
    case 5: return launch_passes<5>(layers, terms, dst, s);
    case 6: return launch_passes<6>(layers, terms, dst, s);
    case 7: return launch_passes<7>(layers, terms, dst, s);
    default: return launch_passes<8>(layers, terms, dst, s);
  }
}

// The margin check of a sightline installation: every shift finite and |shift| <= c_l - 1 (0 when c_l = 0).  shift_host [n_sources][B][2].
int check_shifts(const char* who, int B, int N, const SightSource* sources, int n_sources, const double* shift_host) {
  for (int l = 0; l < n_sources; ++l) {
    const SightSource& y = sources[l];
    const int c = (y.n - N) / 2;
    const double limit = c > 0 ? (double)(c - 1) : 0.0;
    for (size_t i = 0; i < 2 * (size_t)B; ++i) {
      const double v = shift_host[(size_t)l * 2 * B + i];
      if (!std::isfinite(v) || std::fabs(v) > limit)
        return fail(AOG_ERR_INVALID, "%s: shift %c = %.17g pixels of %s %d, env %d is outside the margin (|shift| <= %g: the %s has %d pixels, "
                    "the front %d, c = %d)", who, (i & 1) ? 'y' : 'x', v, y.kind, y.index, (int)(i / 2), limit, y.kind, y.n, N, c);
    }
  }
  return AOG_OK;
}

// The check of a finite-range installation (include/aogym_cone.h): geom_host [n_sources][B][3] = (sx, sy, m); finite, 0 < m <= 1 and on
// each axis |s| + (1 - m) (N - 1) / 2 <= c_l - 1 (one rounded difference, product and sum), which with c_l = 0 leaves s = 0 and m = 1.
int check_cone(const char* who, int B, int N, const SightSource* sources, int n_sources, const double* geom_host) {
  const double ctr = 0.5 * (double)(N - 1);
  for (int l = 0; l < n_sources; ++l) {
    const SightSource& y = sources[l];
    const int c = (y.n - N) / 2;
    const double limit = c > 0 ? (double)(c - 1) : 0.0;
    for (int b = 0; b < B; ++b) {
      const double* g = geom_host + ((size_t)l * B + b) * 3;
      const double m = g[2];
      if (!std::isfinite(m) || !(m > 0.0 && m <= 1.0))
        return fail(AOG_ERR_INVALID, "%s: magnification m = %.17g of %s %d, env %d (0 < m <= 1: m = 1 - altitude / range; margin c = %d)", who, m, y.kind,
                    y.index, b, c);
      const double shrink = (1.0 - m) * ctr;
      for (int a = 0; a < 2; ++a)
        if (!std::isfinite(g[a]) || std::fabs(g[a]) + shrink > limit)
          return fail(AOG_ERR_INVALID, "%s: shift %c = %.17g pixels at m = %.17g of %s %d, env %d is outside the margin (|shift| + (1 - m) (N - 1) / 2 "
                      "<= %g: the %s has %d pixels, the front %d, c = %d)", who, a ? 'y' : 'x', g[a], m, y.kind, y.index, b, limit, y.kind, y.n, N, c);
    }
  }
  return AOG_OK;
}

// The per-(source, env) values of a sightline (`width` 2: shifts) or finite-range (`width` 3: shifts and magnification) installation,
// checked against every source's margin and brought to the front's own buffer on `s`: through pinned staging, which keeps the values of
// the last installation, so that the same values arriving again cost a comparison and no copy.  Nothing of the handle changes before
// every value has passed.
int stage_shifts(const char* who, aog_env* dst, const SightSource* sources, int n_sources, const double* shift_host, int width, hipStream_t s) {
  const size_t B = (size_t)dst->B, count = (size_t)n_sources * B * width;
  if (int rc = width == 3 ? check_cone(who, dst->B, dst->cfg.n_pupil, sources, n_sources, shift_host)
                          : check_shifts(who, dst->B, dst->cfg.n_pupil, sources, n_sources, shift_host))
    return rc;
  const size_t capacity = (size_t)aog::kMaxLayers * B * 3;
  if (!dst->sight_shift)
    if (int rc = dev_alloc(dst, &dst->sight_shift, capacity, false)) return rc;
  if (!dst->sight_stage) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&dst->sight_stage), sizeof(double) * capacity, hipHostMallocDefault));
  if (!dst->sight_ev) HIP_TRY(hipEventCreateWithFlags(&dst->sight_ev, hipEventDisableTiming));
  if (dst->sight_layers == n_sources && dst->sight_width == width && std::memcmp(dst->sight_stage, shift_host, sizeof(double) * count) == 0) return AOG_OK;
  HIP_TRY(hipEventSynchronize(dst->sight_ev));   // (the previous copy out of the staging buffer; long done in practice)
  dst->sight_layers = 0;
  std::memcpy(dst->sight_stage, shift_host, sizeof(double) * count);
  HIP_TRY(hipMemcpyAsync(dst->sight_shift, dst->sight_stage, sizeof(double) * count, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(dst->sight_ev, s));
  dst->sight_layers = n_sources;
  dst->sight_width = width;
  return AOG_OK;
}

// The one installation behind the five entry points; `who` names the entry point in every message.  `shift_host` and the mirrors (sources
// n_layers .. n_layers + n_mirrors - 1, each read as a layer of M pixels whose ring has not turned) belong to the sightline and cone
// forms, `coeff_dev` and `n_terms` to the forms with terms.
int install_layer_sum(const char* who, LayerForm form, aog_env* dst, aog_env* const* layers, int n_layers, const double* shift_host, const double* coeff_dev,
                      int n_terms, void* stream, aog_altmirror* const* mirrors = nullptr, int n_mirrors = 0) {
  const bool cone = form == LayerForm::cone;
  const bool sight = form == LayerForm::sightline || cone;   // (sources larger than the front, terms when n_terms > 0)
  if (sight && n_terms < 0) return fail(AOG_ERR_INVALID, "%s: %d terms", who, n_terms);
  const bool disturbed = sight ? n_terms > 0 : form == LayerForm::disturbed;   // (terms are added)
  if (!dst || !layers || (disturbed && !coeff_dev)) return fail(AOG_ERR_INVALID, "%s: null argument", who);
  if (n_layers < 1 || n_layers > aog::kMaxLayers) return fail(AOG_ERR_INVALID, "%s: %d layers (1 .. %d)", who, n_layers, aog::kMaxLayers);
  if (n_mirrors < 0 || n_layers + n_mirrors > aog::kMaxLayers || (n_mirrors > 0 && !mirrors))
    return fail(AOG_ERR_INVALID, "%s: %d layers and %d mirrors (n_mirrors >= 0 with its array, together at most %d sources)", who, n_layers, n_mirrors,
                aog::kMaxLayers);
  const int n_sources = n_layers + n_mirrors;
  SightSource sources[aog::kMaxLayers];
  if (dst->cfg.atm_dynamic) return fail(AOG_ERR_INVALID, "%s: the front handle must not be atm_dynamic (its screens are installed, not evolved)", who);
  if (!dst->tables_ready) return fail(AOG_ERR_INVALID, "%s before aog_upload_tables", who);
  if (disturbed && !dst->dist_basis) return fail(AOG_ERR_INVALID, "%s before aog_upload_disturbance_basis", who);
  if (disturbed && n_terms != dst->dist_terms)
    return fail(AOG_ERR_INVALID, "%s: %d terms of coefficients, the uploaded basis has %d", who, n_terms, dst->dist_terms);
  aog::LayerSources src{};
  for (int l = 0; l < n_layers; ++l) {
    const aog_env* y = layers[l];
    if (!y) return fail(AOG_ERR_INVALID, "%s: layer %d is null", who, l);
    if (!y->cfg.atm_dynamic || !y->screens_ready || !y->psi_master) return fail(AOG_ERR_INVALID, "%s: layer %d is not a dynamic handle with screens", who, l);
    const bool n_ok = sight ? y->cfg.n_pupil >= dst->cfg.n_pupil : y->cfg.n_pupil == dst->cfg.n_pupil;
    if (y->device != dst->device || !n_ok || y->B != dst->B || y->cfg.env_id_base != dst->cfg.env_id_base)
      return fail(AOG_ERR_INVALID, "%s: layer %d (device %d, N %d, B %d, env_id_base %d) does not match the front handle (device %d, N %d, B %d, "
                  "env_id_base %d)", who, l, y->device, y->cfg.n_pupil, y->B, y->cfg.env_id_base, dst->device, dst->cfg.n_pupil, dst->B, dst->cfg.env_id_base);
    if (sight && (y->cfg.n_pupil - dst->cfg.n_pupil) % 2)
      return fail(AOG_ERR_INVALID, "%s: layer %d has %d pixels, the front %d: the difference must be even (the meta-pupil is centred on the pupil)", who, l,
                  y->cfg.n_pupil, dst->cfg.n_pupil);
    if (y->pre_evolved) return fail(AOG_ERR_INVALID, "%s: the atmosphere of layer %d already stands at the next step (aog_set_lookahead)", who, l);
    char layer_who[96];
    std::snprintf(layer_who, sizeof layer_who, "%s (layer)", who);
    if (int rc = check_poisoned(y, layer_who)) return rc;
    src.master[l] = y->psi_master;
    src.origin[l] = y->origin;
    sources[l] = {"layer", l, y->cfg.n_pupil};
  }
  for (int j = 0; j < n_mirrors; ++j) {
    const aog_altmirror* m = mirrors[j];
    if (!m) return fail(AOG_ERR_INVALID, "%s: mirror %d is null", who, j);
    const int M = m->cfg.n_pixels;
    if (m->state.device != dst->device || m->cfg.num_envs != dst->B || M < dst->cfg.n_pupil)
      return fail(AOG_ERR_INVALID, "%s: mirror %d (device %d, n_pixels %d, num_envs %d) does not match the front handle (device %d, N %d, B %d)", who, j,
                  m->state.device, M, m->cfg.num_envs, dst->device, dst->cfg.n_pupil, dst->B);
    if ((M - dst->cfg.n_pupil) % 2)
      return fail(AOG_ERR_INVALID, "%s: mirror %d has %d pixels, the front %d: the difference must be even (the meta-pupil is centred on the pupil)", who,
                  j, M, dst->cfg.n_pupil);
    src.master[n_layers + j] = m->surface;
    src.origin[n_layers + j] = m->origin;
    sources[n_layers + j] = {"mirror", j, M};
  }
  const bool fast = dst->cfg.precision == AOG_PRECISION_FAST;
  if (fast && dst->kernel != AOG_KERNEL_MFMA)
    return fail(AOG_ERR_UNSUPPORTED, "%s: the front handle runs the VALU kernel (its screen layout is not written here; use kernel 'auto' or 'mfma')", who);
  if (int rc = check_poisoned(dst, who)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (sight)
    if (int rc = stage_shifts(who, dst, sources, n_sources, shift_host, cone ? 3 : 2, s)) return rc;
  if (!dst->layer_mean)
    if (int rc = dev_alloc(dst, &dst->layer_mean, (size_t)dst->B, false)) return rc;
  const aog::ModalTerms terms{disturbed ? dst->dist_basis : nullptr, disturbed ? coeff_dev : nullptr, disturbed ? n_terms : 0, dst->n_ap};
  if (cone) {
    aog::ConeLayers seen{src, {}};
    for (int l = 0; l < n_sources; ++l) {
      seen.cone.geom[l] = dst->sight_shift + (size_t)l * dst->B * 3;
      seen.cone.n[l] = sources[l].n;
      seen.cone.c[l] = (sources[l].n - dst->cfg.n_pupil) / 2;
    }
    launch_passes(n_sources, seen, terms, dst, s);
  } else if (sight) {
    aog::SightLayers seen{src, {}};
    for (int l = 0; l < n_sources; ++l) {
      seen.sight.shift[l] = dst->sight_shift + (size_t)l * dst->B * 2;
      seen.sight.n[l] = sources[l].n;
      seen.sight.c[l] = (sources[l].n - dst->cfg.n_pupil) / 2;
    }
    launch_passes(n_sources, seen, terms, dst, s);
  } else if (disturbed) {
    launch_passes(n_layers, src, terms, dst, s);
  } else {
    launch_passes(n_layers, src, aog::NoTerms{}, dst, s);
  }
  HIP_TRY(hipGetLastError());
  dst->screens_ready = true;
  dst->reset_obs_valid = false;   // new screens: the kept reset observation is of the old ones
  dst->sh_sums_ready = false;
  return AOG_OK;
}

}  // namespace

extern "C" {

int aog_evolve_atmosphere(aog_env* e, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_evolve_atmosphere: null handle");
  if (!e->cfg.atm_dynamic) return fail(AOG_ERR_STATE, "aog_evolve_atmosphere: handle was not created with atm_dynamic = 1");
  if (!e->layer_ready) return fail(AOG_ERR_STATE, "aog_evolve_atmosphere: aog_upload_layer / aog_set_wind not called");
  if (!e->screens_ready) return fail(AOG_ERR_STATE, "aog_evolve_atmosphere before any screen was installed");
  if (e->lookahead) return fail(AOG_ERR_STATE, "aog_evolve_atmosphere: not together with aog_set_lookahead (aog_step evolves such a handle ahead of time)");
  if (int rc = refuse_pre_evolved(e, "aog_evolve_atmosphere")) return rc;
  if (int rc = check_poisoned(e, "aog_evolve_atmosphere")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  e->timestep += 1;   // as step_body: from here on a failure leaves counters and ring out of step with each other
  e->steps_since_reset += 1;
  e->sh_sums_ready = false;
  const int rc = evolve_layer(e, static_cast<hipStream_t>(stream), e->timestep);
  if (rc != AOG_OK) poison(e, 2);
  return rc;
}

int aog_install_layer_sum(aog_env* dst, aog_env* const* layers, int n_layers, void* stream) {
  return install_layer_sum("aog_install_layer_sum", LayerForm::plain, dst, layers, n_layers, nullptr, nullptr, 0, stream);
}

int aog_upload_disturbance_basis(aog_env* dst, const double* basis_host, int n_terms) {
  if (!dst || !basis_host) return fail(AOG_ERR_INVALID, "aog_upload_disturbance_basis: null argument");
  if (n_terms < 1 || n_terms > aog::kMaxTerms) return fail(AOG_ERR_INVALID, "aog_upload_disturbance_basis: %d terms (1 .. %d)", n_terms, aog::kMaxTerms);
  if (!dst->tables_ready) return fail(AOG_ERR_INVALID, "aog_upload_disturbance_basis before aog_upload_tables");
  const size_t count = (size_t)n_terms * dst->n_ap;
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(basis_host[i]))
      return fail(AOG_ERR_INVALID, "aog_upload_disturbance_basis: term %d is not finite at aperture pixel %d", (int)(i / dst->n_ap), (int)(i % dst->n_ap));
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());   // (an installation that reads the basis being replaced may still be queued)
  if (dst->dist_basis && dst->dist_terms != n_terms) dev_release(dst, &dst->dist_basis);
  dst->dist_terms = 0;
  if (int rc = upload(dst, &dst->dist_basis, basis_host, count, true)) return rc;
  dst->dist_terms = n_terms;
  return AOG_OK;
}

int aog_install_layer_sum_disturbed(aog_env* dst, aog_env* const* layers, int n_layers, const double* coeff_dev, int n_terms, void* stream) {
  return install_layer_sum("aog_install_layer_sum_disturbed", LayerForm::disturbed, dst, layers, n_layers, nullptr, coeff_dev, n_terms, stream);
}

int aog_install_layer_sum_sightline(aog_env* dst, aog_env* const* layers, int n_layers, const double* shift_host, const double* coeff_dev, int n_terms,
                                    void* stream) {
  if (!shift_host) return fail(AOG_ERR_INVALID, "aog_install_layer_sum_sightline: null argument");
  return install_layer_sum("aog_install_layer_sum_sightline", LayerForm::sightline, dst, layers, n_layers, shift_host, coeff_dev, n_terms, stream);
}

int aog_install_layer_sum_conjugate(aog_env* dst, aog_env* const* layers, int n_layers, aog_altmirror* const* mirrors, int n_mirrors,
                                    const double* shift_host, const double* coeff_dev, int n_terms, void* stream) {
  if (!shift_host) return fail(AOG_ERR_INVALID, "aog_install_layer_sum_conjugate: null argument");
  return install_layer_sum("aog_install_layer_sum_conjugate", LayerForm::sightline, dst, layers, n_layers, shift_host, coeff_dev, n_terms, stream, mirrors,
                           n_mirrors);
}

int aog_install_layer_sum_cone(aog_env* dst, aog_env* const* layers, int n_layers, aog_altmirror* const* mirrors, int n_mirrors, const double* geom_host,
                               const double* coeff_dev, int n_terms, void* stream) {
  if (!geom_host) return fail(AOG_ERR_INVALID, "aog_install_layer_sum_cone: null argument");
  return install_layer_sum("aog_install_layer_sum_cone", LayerForm::cone, dst, layers, n_layers, geom_host, coeff_dev, n_terms, stream, mirrors, n_mirrors);
}

int aog_cone_check_geometry(const double* geom_host, int n_layers, int n_mirrors, int num_envs, int n_pupil, const int32_t* source_pixels) {
  const char* who = "aog_cone_check_geometry";
  if (!geom_host || !source_pixels) return fail(AOG_ERR_INVALID, "%s: null argument", who);
  if (n_layers < 1 || n_mirrors < 0 || n_layers + n_mirrors > aog::kMaxLayers)
    return fail(AOG_ERR_INVALID, "%s: %d layers and %d mirrors (n_layers >= 1, n_mirrors >= 0, together at most %d sources)", who, n_layers, n_mirrors,
                aog::kMaxLayers);
  if (num_envs < 1 || n_pupil < 1) return fail(AOG_ERR_INVALID, "%s: num_envs %d, n_pupil %d (each >= 1)", who, num_envs, n_pupil);
  SightSource sources[aog::kMaxLayers];
  for (int l = 0; l < n_layers + n_mirrors; ++l) {
    sources[l] = l < n_layers ? SightSource{"layer", l, source_pixels[l]} : SightSource{"mirror", l - n_layers, source_pixels[l]};
    if (source_pixels[l] < n_pupil || (source_pixels[l] - n_pupil) % 2)
      return fail(AOG_ERR_INVALID, "%s: %s %d has %d pixels, the front %d: at least as many, the difference even (the meta-pupil is centred on the "
                  "pupil)", who, sources[l].kind, sources[l].index, source_pixels[l], n_pupil);
  }
  return check_cone(who, num_envs, n_pupil, sources, n_layers + n_mirrors, geom_host);
}

}  // extern "C"
