// K26: scintillation (aog_scint_*): the Fresnel filter of the layers above the ground (hipFFT between hand-written pack, multiply and unpack),
// the installation of a front's log-amplitude map and the amplitude-aware receiver.  A translation unit of its own: no kernel a step
// launches changes.
#include "conjugate_host.h"
#include "k_scintillation.h"
#include "../../include/aogym_scintillation.h"

#include <hipfft/hipfft.h>

using namespace aog_host;

static_assert(aog::kScintFiber == AOG_SCINT_MAX_FIBER && aog::kMaxLayers == AOG_SCINT_MAX_LAYERS, "the header's limits");

struct aog_scint : StandaloneHandle<aog_scint_config> {   // no state: chi is a function of the layers' screens
  double* filter = nullptr;    // [L][E][E][2]
  double* corr = nullptr;      // [L][B][M M]
  double* chi = nullptr;       // [L][B][M M]
  double* work = nullptr;      // [chunk][E][E][2]
  int32_t* origin = nullptr;   // [B][2] zeros
  double* wmodes = nullptr;    // [n_ptiles 32][4][2]
  double* slabs = nullptr;     // [n_chunks][kScintRows][Bp]
  size_t wmodes_rows = 0, slab_count = 0;
  int chunk = 0;
  hipfftHandle plan = 0, plan_tail = 0;   // batch = chunk, batch = B % chunk (0: none)
  size_t plan_bytes = 0;
  bool has_filter = false, filtered = false;
  std::vector<aog_altmirror> views;   // one per layer: corr[l] as an altitude mirror's surface (nothing owned)
};

namespace {

size_t mm(const aog_scint* s) { return (size_t)s->cfg.n_pixels * s->cfg.n_pixels; }
size_t ee(const aog_scint* s) { return 4 * mm(s); }

int scint_check(const aog_scint_config* cfg) {
  const char* who = "aog_scint_create";
  if (cfg->abi_version != AOG_ABI_VERSION) return fail(AOG_ERR_INVALID, "%s: abi_version %d, the library is %d", who, cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "%s: num_envs %d must be >= 1", who, cfg->num_envs);
  if (cfg->n_pixels < 2 || cfg->n_pixels > 8192) return fail(AOG_ERR_INVALID, "%s: n_pixels %d outside [2, 8192]", who, cfg->n_pixels);
  if (cfg->n_layers < 0 || cfg->n_layers > AOG_SCINT_MAX_LAYERS) return fail(AOG_ERR_INVALID, "%s: n_layers %d outside [0, %d]", who, cfg->n_layers, AOG_SCINT_MAX_LAYERS);
  if (cfg->n_fiber < 1 || cfg->n_fiber > AOG_SCINT_MAX_FIBER) return fail(AOG_ERR_INVALID, "%s: n_fiber %d outside [1, %d]", who, cfg->n_fiber, AOG_SCINT_MAX_FIBER);
  if (cfg->reserved != 0) return fail(AOG_ERR_INVALID, "%s: reserved must be 0", who);
  if (cfg->scratch_bytes < 1) return fail(AOG_ERR_INVALID, "%s: scratch_bytes must be > 0", who);
  // (the kernels number pixels with 32-bit integers)
  if ((long long)cfg->num_envs * cfg->n_pixels * cfg->n_pixels > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "%s: num_envs %d x n_pixels %d^2 exceeds 2^31 - 1 surface values", who, cfg->num_envs, cfg->n_pixels);
  return AOG_OK;
}

hipError_t make_plan(aog_scint* s, hipfftHandle* plan, int batch) {
  int dims[2] = {2 * s->cfg.n_pixels, 2 * s->cfg.n_pixels};
  const int dist = (int)ee(s);
  if (hipfftPlanMany(plan, 2, dims, nullptr, 1, dist, nullptr, 1, dist, HIPFFT_Z2Z, batch) != HIPFFT_SUCCESS) return hipErrorUnknown;
  size_t bytes = 0;
  if (hipfftGetSize(*plan, &bytes) == HIPFFT_SUCCESS) s->plan_bytes = std::max(s->plan_bytes, bytes);
  return hipSuccess;
}

// a fast MFMA front of the handle's batch and device, tables and screens there
int front_check(const char* who, const aog_scint* s, const aog_env* e) {
  if (e->device != s->state.device || e->B != s->cfg.num_envs || e->cfg.n_pupil > s->cfg.n_pixels || (s->cfg.n_pixels - e->cfg.n_pupil) % 2)
    return fail(AOG_ERR_INVALID, "%s: the front (device %d, N %d, B %d) does not match the handle (device %d, n_pixels %d >= N with an even difference, "
                "num_envs %d)", who, e->device, e->cfg.n_pupil, e->B, s->state.device, s->cfg.n_pixels, s->cfg.num_envs);
  if (!e->tables_ready) return fail(AOG_ERR_INVALID, "%s before aog_upload_tables", who);
  if (e->cfg.precision != AOG_PRECISION_FAST || e->kernel != AOG_KERNEL_MFMA || !e->psi_tile)
    return fail(AOG_ERR_UNSUPPORTED, "%s: the front is not a fast handle on the MFMA kernel (the log-amplitude map and the receiver are built on its screen "
                "tiles)", who);
  return AOG_OK;
}

template <typename F>
void with_layers(int L, F&& f) {
  switch (L) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace

extern "C" {

int64_t aog_scint_config_size(void) { return (int64_t)sizeof(aog_scint_config); }

int aog_scint_create(const aog_scint_config* cfg, int device, aog_scint** out) {
  return handle_create("aog_scint_create", cfg, device, out, scint_check, [](aog_scint* s) {
    const size_t L = (size_t)s->cfg.n_layers, B = (size_t)s->cfg.num_envs;
    const size_t per_env = sizeof(double) * 2 * ee(s);
    s->chunk = (int)std::max<size_t>(1, std::min<size_t>(B, (size_t)s->cfg.scratch_bytes / per_env));
    if (L == 0) return hipSuccess;   // every layer on the ground: a receiver only, nothing to filter
    if (hipError_t err = s->own(&s->filter, sizeof(double) * 2 * L * ee(s), true)) return err;
    if (hipError_t err = s->own(&s->corr, sizeof(double) * L * B * mm(s), true)) return err;
    if (hipError_t err = s->own(&s->chi, sizeof(double) * L * B * mm(s), true)) return err;
    if (hipError_t err = s->own(&s->work, per_env * s->chunk, false)) return err;
    if (hipError_t err = s->own(&s->origin, sizeof(int32_t) * B * 2, true)) return err;
    if (hipError_t err = make_plan(s, &s->plan, s->chunk)) return err;
    if (B % s->chunk)
      if (hipError_t err = make_plan(s, &s->plan_tail, (int)(B % s->chunk))) return err;
    s->views.resize(L);
    for (size_t l = 0; l < L; ++l) {
      aog_altmirror& v = s->views[l];
      v.cfg = aog_altmirror_config{AOG_ABI_VERSION, s->cfg.num_envs, s->cfg.n_pixels, 1, 0};
      v.state.device = s->state.device;
      v.surface = s->corr + l * B * mm(s);
      v.origin = s->origin;
    }
    return hipSuccess;
  });
}

void aog_scint_destroy(aog_scint* s) {
  if (!s) return;
  (void)hipSetDevice(s->state.device);
  (void)hipDeviceSynchronize();   // (hipFFT's work areas go with the plans)
  if (s->plan) hipfftDestroy(s->plan);
  if (s->plan_tail) hipfftDestroy(s->plan_tail);
  handle_destroy(s);
}

int aog_scint_upload(aog_scint* s, const double* filter_dev, void* stream) {
  REFUSE_NULL("aog_scint_upload", {"scint", s}, {"filter_dev", filter_dev});
  if (s->cfg.n_layers == 0) return fail(AOG_ERR_INVALID, "aog_scint_upload: the handle has no layer to filter");
  HIP_TRY(hipSetDevice(s->state.device));
  HIP_TRY(hipMemcpyAsync(s->filter, filter_dev, sizeof(double) * 2 * s->cfg.n_layers * ee(s), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  s->has_filter = true;
  return AOG_OK;
}

int aog_scint_upload_modes(aog_scint* s, aog_env* front, const double* modes_host) {
  const char* who = "aog_scint_upload_modes";
  REFUSE_NULL(who, {"scint", s}, {"front", front}, {"modes_host", modes_host});
  if (int rc = front_check(who, s, front)) return rc;
  HIP_TRY(hipSetDevice(s->state.device));
  const size_t rows = (size_t)front->n_ptiles * 32;
  if (s->wmodes && s->wmodes_rows != rows) return fail(AOG_ERR_INVALID, "%s: the handle holds modes of %zu pixel slots, this front has %zu", who, s->wmodes_rows, rows);
  std::vector<double> table(rows * aog::kScintFiber * 2, 0.0);
  for (int k = 0; k < s->cfg.n_fiber; ++k)
    for (int p = 0; p < front->n_ap; ++p) {
      const double re = modes_host[((size_t)k * front->n_ap + p) * 2], im = modes_host[((size_t)k * front->n_ap + p) * 2 + 1];
      if (!std::isfinite(re) || !std::isfinite(im)) return fail(AOG_ERR_INVALID, "%s: mode %d is not finite at aperture pixel %d", who, k, p);
      table[((size_t)p * aog::kScintFiber + k) * 2] = re;
      table[((size_t)p * aog::kScintFiber + k) * 2 + 1] = im;
    }
  HIP_TRY(hipDeviceSynchronize());   // (a receiver that reads the table being replaced may still be queued)
  if (!s->wmodes) HIP_TRY(s->own(&s->wmodes, sizeof(double) * table.size(), false));
  s->wmodes_rows = rows;
  HIP_TRY(hipMemcpy(s->wmodes, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice));
  return AOG_OK;
}

int aog_scint_filter(aog_scint* s, aog_env* const* layers, void* stream) {
  const char* who = "aog_scint_filter";
  REFUSE_NULL(who, {"scint", s}, {"layers", layers});
  if (s->cfg.n_layers == 0) return AOG_OK;
  if (!s->has_filter) return fail(AOG_ERR_INVALID, "%s before aog_scint_upload", who);
  const int L = s->cfg.n_layers, B = s->cfg.num_envs, M = s->cfg.n_pixels;
  for (int l = 0; l < L; ++l) {
    const aog_env* y = layers[l];
    if (!y) return fail(AOG_ERR_INVALID, "%s: layer %d is null", who, l);
    if (!y->cfg.atm_dynamic || !y->screens_ready || !y->psi_master) return fail(AOG_ERR_INVALID, "%s: layer %d is not a dynamic handle with screens", who, l);
    if (y->device != s->state.device || y->cfg.n_pupil != M || y->B != B)
      return fail(AOG_ERR_INVALID, "%s: layer %d (device %d, N %d, B %d) does not match the handle (device %d, n_pixels %d, num_envs %d)", who, l, y->device,
                  y->cfg.n_pupil, y->B, s->state.device, M, B);
    if (int rc = refuse_pre_evolved(y, who)) return rc;
    if (int rc = check_poisoned(y, "aog_scint_filter (layer)")) return rc;
  }
  HIP_TRY(hipSetDevice(s->state.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int EE = (int)ee(s);
  const double inv_n = 1.0 / (double)EE;
  for (int env0 = 0; env0 < B; env0 += s->chunk) {
    const int n = std::min(s->chunk, B - env0);
    hipfftHandle plan = n == s->chunk ? s->plan : s->plan_tail;
    if (hipfftSetStream(plan, st) != HIPFFT_SUCCESS) return fail(AOG_ERR_HIP, "%s: hipfftSetStream failed", who);
    hipfftDoubleComplex* buf = reinterpret_cast<hipfftDoubleComplex*>(s->work);
    for (int l = 0; l < L; ++l) {
      const aog_env* y = layers[l];
      hipLaunchKernelGGL(aog::k_scint_pack, dim3((EE + 255) / 256, n), dim3(256), 0, st, y->psi_master, y->origin, reinterpret_cast<double2*>(s->work), env0, M);
      HIP_TRY(hipGetLastError());
      if (hipfftExecZ2Z(plan, buf, buf, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail(AOG_ERR_HIP, "%s: hipfftExecZ2Z forward failed", who);
      hipLaunchKernelGGL(aog::k_scint_multiply, dim3((EE + 255) / 256, n), dim3(256), 0, st, reinterpret_cast<const double2*>(s->filter) + (size_t)l * EE,
                         reinterpret_cast<double2*>(s->work), EE);
      HIP_TRY(hipGetLastError());
      if (hipfftExecZ2Z(plan, buf, buf, HIPFFT_BACKWARD) != HIPFFT_SUCCESS) return fail(AOG_ERR_HIP, "%s: hipfftExecZ2Z backward failed", who);
      hipLaunchKernelGGL(aog::k_scint_unpack, dim3((M * M + 255) / 256, n), dim3(256), 0, st, reinterpret_cast<const double2*>(s->work), y->psi_master, y->origin,
                         s->corr + (size_t)l * B * mm(s), s->chi + (size_t)l * B * mm(s), env0, M, inv_n);
      HIP_TRY(hipGetLastError());
    }
  }
  s->filtered = true;
  return AOG_OK;
}

aog_altmirror* aog_scint_correction(aog_scint* s, int layer) {
  if (!s || layer < 0 || layer >= s->cfg.n_layers) {
    fail(AOG_ERR_INVALID, "aog_scint_correction: null handle or layer %d outside the handle's layers", layer);
    return nullptr;
  }
  return &s->views[(size_t)layer];
}

int aog_scint_get(aog_scint* s, int layer, double* corr_out, double* chi_out, void* stream) {
  REFUSE_NULL("aog_scint_get", {"scint", s});
  if (layer < 0 || layer >= s->cfg.n_layers) return fail(AOG_ERR_INVALID, "aog_scint_get: layer %d outside [0, %d)", layer, s->cfg.n_layers);
  HIP_TRY(hipSetDevice(s->state.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t count = (size_t)s->cfg.num_envs * mm(s);
  if (corr_out) HIP_TRY(hipMemcpyAsync(corr_out, s->corr + layer * count, sizeof(double) * count, hipMemcpyDeviceToDevice, st));
  if (chi_out) HIP_TRY(hipMemcpyAsync(chi_out, s->chi + layer * count, sizeof(double) * count, hipMemcpyDeviceToDevice, st));
  return AOG_OK;
}

int64_t aog_scint_tile_floats(const aog_env* front) { return front ? (int64_t)front->n_etiles * front->n_ptiles * 1024 : 0; }

int64_t aog_scint_scratch_bytes(const aog_scint* s) { return s && s->work ? (int64_t)(sizeof(double) * 2 * ee(s) * s->chunk + s->plan_bytes) : 0; }

int aog_scint_install(aog_scint* s, aog_env* front, const double* shift_host, const double* shift_dev, float* chi_tile_dev, void* stream) {
  const char* who = "aog_scint_install";
  REFUSE_NULL(who, {"scint", s}, {"front", front}, {"shift_host", shift_host}, {"shift_dev", shift_dev}, {"chi_tile_dev", chi_tile_dev});
  if (int rc = front_check(who, s, front)) return rc;
  if (!s->filtered || s->cfg.n_layers == 0) return fail(AOG_ERR_INVALID, "%s before aog_scint_filter (or on a handle without layers)", who);
  const int L = s->cfg.n_layers, B = s->cfg.num_envs, M = s->cfg.n_pixels, N = front->cfg.n_pupil;
  const int c = (M - N) / 2;
  const double limit = c > 0 ? (double)(c - 1) : 0.0;
  const size_t count = (size_t)L * B * 2;
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(shift_host[i]) || std::fabs(shift_host[i]) > limit)
      return fail(AOG_ERR_INVALID, "%s: shift %c = %.17g pixels of layer %d, env %d is outside the margin (|shift| <= %g, c = %d)", who, (i & 1) ? 'y' : 'x',
                  shift_host[i], (int)(i / (2 * (size_t)B)), (int)((i / 2) % B), limit, c);
  HIP_TRY(hipSetDevice(s->state.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  aog::SightLayers chi{};
  for (int l = 0; l < L; ++l) {
    chi.master[l] = s->chi + (size_t)l * B * mm(s);
    chi.origin[l] = s->origin;
    chi.sight.shift[l] = shift_dev + (size_t)l * B * 2;
    chi.sight.n[l] = M;
    chi.sight.c[l] = c;
  }
  const dim3 grid((unsigned)((front->n_ptiles * 32 + 255) / 256), (unsigned)(front->n_etiles * 32));
  with_layers(L, [&](auto nl) {
    hipLaunchKernelGGL((aog::k_scint_install<nl()>), grid, dim3(256), 0, st, chi, front->ap_index, chi_tile_dev, B, N, front->n_ap, front->n_ptiles,
                       1.0 / front->cfg.wavelength_wfs);
  });
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_scint_receive(aog_scint* s, aog_env* e, const float* chi_tile_dev, double* power_dev, double* irradiance_dev, double* strehl_dev, double* sigma_chi2_dev,
                      void* stream) {
  const char* who = "aog_scint_receive";
  REFUSE_NULL(who, {"scint", s}, {"front", e});
  if (!power_dev && !irradiance_dev && !strehl_dev && !sigma_chi2_dev) return fail(AOG_ERR_INVALID, "%s: every output pointer is null", who);
  if (int rc = front_check(who, s, e)) return rc;
  if (int rc = instrument_gate(e, who, s->wmodes != nullptr && s->wmodes_rows == (size_t)e->n_ptiles * 32, "the receive modes were", "aog_scint_upload_modes")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n_chunks = aog::pupil_chunks(e->n_ptiles);
  const size_t need_count = (size_t)n_chunks * aog::kScintRows * e->Bp;
  if (!s->slabs) {
    HIP_TRY(s->own(&s->slabs, sizeof(double) * need_count, false));
    s->slab_count = need_count;
  }
  if (s->slab_count != need_count) return fail(AOG_ERR_INVALID, "%s: the handle's slabs were sized for another front", who);
  if (int rc = instrument_operands(e, st, false)) return rc;
  with_apad(e->A_pad, [&](auto apad) {
    hipLaunchKernelGGL((aog::k_scint_receive<apad()>), dim3(n_chunks, e->n_etiles), dim3(256), 0, st, reinterpret_cast<const aog::f16x8*>(e->modes16),
                       reinterpret_cast<const aog::f32x4*>(e->psi_tile), reinterpret_cast<const aog::f16x8*>(e->inst_act16),
                       reinterpret_cast<const aog::f32x4*>(chi_tile_dev), reinterpret_cast<const double2*>(s->wmodes), s->slabs, e->n_ptiles, e->n_ap, e->Bp);
  });
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(aog::k_scint_finish, dim3((e->B + 255) / 256), dim3(256), 0, st, s->slabs, n_chunks, e->Bp, e->B, e->n_ap, power_dev, irradiance_dev,
                     strehl_dev, sigma_chi2_dev);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

}  // extern "C"
