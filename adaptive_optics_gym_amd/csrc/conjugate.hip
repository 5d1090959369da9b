// K23: the altitude-conjugated deformable mirror (aog_altmirror_*): a command becomes a surface on the meta-pupil, which
// aog_install_layer_sum_conjugate (layers.hip) reads beside the layers; a layer's screen becomes its best-fit command.
#include "conjugate_host.h"
#include "k_conjugate.h"

using namespace aog_host;

namespace {

size_t envs(const aog_altmirror* m) { return (size_t)m->cfg.num_envs; }
size_t modes(const aog_altmirror* m) { return (size_t)m->cfg.n_modes; }
size_t pixels(const aog_altmirror* m) { return (size_t)m->cfg.n_pixels * m->cfg.n_pixels; }
double* record(const aog_altmirror* m) { return reinterpret_cast<double*>(m->state.ptr); }

int altmirror_check(const aog_altmirror_config* cfg) {
  if (cfg->abi_version != AOG_ABI_VERSION)
    return fail(AOG_ERR_INVALID, "aog_altmirror_create: abi_version %d, the library is %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(AOG_ERR_INVALID, "aog_altmirror_create: num_envs %d must be >= 1", cfg->num_envs);
  if (cfg->n_pixels < 1) return fail(AOG_ERR_INVALID, "aog_altmirror_create: n_pixels %d must be >= 1", cfg->n_pixels);
  if (cfg->n_modes < 1 || cfg->n_modes > AOG_ALTMIRROR_MAX_MODES)
    return fail(AOG_ERR_INVALID, "aog_altmirror_create: n_modes %d outside [1, %d]", cfg->n_modes, AOG_ALTMIRROR_MAX_MODES);
  if (cfg->reserved != 0) return fail(AOG_ERR_INVALID, "aog_altmirror_create: reserved must be 0");
  // (the kernels number pixels and workgroups with 32-bit integers)
  if ((long long)cfg->num_envs * cfg->n_pixels * cfg->n_pixels > 0x7FFFFFFFll)
    return fail(AOG_ERR_INVALID, "aog_altmirror_create: num_envs %d x n_pixels %d^2 exceeds 2^31 - 1 surface values", cfg->num_envs, cfg->n_pixels);
  return AOG_OK;
}

// the one launch of kernel 1: the surfaces of the envs `mask` selects from `cmd`, which also goes to the record unless it is the record
int synthesise(aog_altmirror* m, const double* cmd, const uint8_t* mask, void* stream) {
  const int B = m->cfg.num_envs, MM = (int)pixels(m);
  const int n_groups = (B + aog::kSurfEnvs - 1) / aog::kSurfEnvs, n_chunks = (MM + aog::kSurfPixels - 1) / aog::kSurfPixels;
  LAUNCH_PLAIN(m->state.device, stream, aog::k_altmirror_surface, dim3((unsigned)n_groups * (unsigned)n_chunks), dim3(256), m->basis, cmd, mask,
               cmd == record(m) ? nullptr : record(m), m->surface, B, m->cfg.n_modes, MM, n_groups);
  return AOG_OK;
}

}  // namespace

extern "C" {

int64_t aog_altmirror_config_size(void) { return (int64_t)sizeof(aog_altmirror_config); }

int aog_altmirror_create(const aog_altmirror_config* cfg, int device, aog_altmirror** out) {
  // commands, surfaces, origins and the basis start as zeros
  return handle_create("aog_altmirror_create", cfg, device, out, altmirror_check, [](aog_altmirror* m) {
    if (hipError_t err = m->alloc_state(sizeof(double) * envs(m) * modes(m), true)) return err;
    if (hipError_t err = m->own(&m->basis, sizeof(double) * modes(m) * pixels(m), true)) return err;
    if (hipError_t err = m->own(&m->surface, sizeof(double) * envs(m) * pixels(m), true)) return err;
    return m->own(&m->origin, sizeof(int32_t) * envs(m) * 2, true);
  });
}

void aog_altmirror_destroy(aog_altmirror* m) { handle_destroy(m); }

int aog_altmirror_upload(aog_altmirror* m, const double* basis_dev, const double* fit_dev, void* stream) {
  REFUSE_NULL("aog_altmirror_upload", {"mirror", m}, {"basis_dev", basis_dev});
  HIP_TRY(hipSetDevice(m->state.device));
  const size_t bytes = sizeof(double) * modes(m) * pixels(m);
  hipStream_t s = static_cast<hipStream_t>(stream);
  m->has_fit = false;
  if (fit_dev && !m->fit) HIP_TRY(m->own(&m->fit, bytes, false));
  HIP_TRY(hipMemcpyAsync(m->basis, basis_dev, bytes, hipMemcpyDeviceToDevice, s));
  if (fit_dev) {
    HIP_TRY(hipMemcpyAsync(m->fit, fit_dev, bytes, hipMemcpyDeviceToDevice, s));
    m->has_fit = true;
  }
  return AOG_OK;
}

int aog_altmirror_set_command(aog_altmirror* m, const double* cmd_dev, const uint8_t* mask_dev, void* stream) {
  REFUSE_NULL("aog_altmirror_set_command", {"mirror", m}, {"cmd_dev", cmd_dev});
  return synthesise(m, cmd_dev, mask_dev, stream);
}

int aog_altmirror_get(aog_altmirror* m, double* cmd_out, double* surface_out, void* stream) {
  REFUSE_NULL("aog_altmirror_get", {"mirror", m});
  HIP_TRY(hipSetDevice(m->state.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (cmd_out) HIP_TRY(hipMemcpyAsync(cmd_out, record(m), sizeof(double) * envs(m) * modes(m), hipMemcpyDeviceToDevice, s));
  if (surface_out) HIP_TRY(hipMemcpyAsync(surface_out, m->surface, sizeof(double) * envs(m) * pixels(m), hipMemcpyDeviceToDevice, s));
  return AOG_OK;
}

int aog_altmirror_fit(aog_altmirror* m, aog_env* layer, double* cmd_out, void* stream) {
  REFUSE_NULL("aog_altmirror_fit", {"mirror", m}, {"layer", layer}, {"cmd_out", cmd_out});
  if (!m->has_fit) return fail(AOG_ERR_INVALID, "aog_altmirror_fit: no fit matrix was uploaded (aog_altmirror_upload with fit_dev)");
  if (!layer->cfg.atm_dynamic || !layer->screens_ready || !layer->psi_master)
    return fail(AOG_ERR_INVALID, "aog_altmirror_fit: the layer is not a dynamic handle with screens");
  if (layer->device != m->state.device || layer->cfg.n_pupil != m->cfg.n_pixels || layer->B != m->cfg.num_envs)
    return fail(AOG_ERR_INVALID, "aog_altmirror_fit: the layer (device %d, N %d, B %d) does not match the mirror (device %d, n_pixels %d, num_envs %d)",
                layer->device, layer->cfg.n_pupil, layer->B, m->state.device, m->cfg.n_pixels, m->cfg.num_envs);
  if (int rc = refuse_pre_evolved(layer, "aog_altmirror_fit")) return rc;
  if (int rc = check_poisoned(layer, "aog_altmirror_fit (layer)")) return rc;
  const dim3 grid((unsigned)m->cfg.num_envs, (unsigned)((m->cfg.n_modes + aog::kFitModes - 1) / aog::kFitModes));
  LAUNCH_PLAIN(m->state.device, stream, aog::k_altmirror_fit, grid, dim3(256), m->fit, layer->psi_master, layer->origin, cmd_out, m->cfg.n_modes,
               m->cfg.n_pixels);
  return AOG_OK;
}

int64_t aog_altmirror_state_bytes(const aog_altmirror* m) { return handle_state_bytes(m); }

int aog_altmirror_get_state(aog_altmirror* m, void* blob_dev, void* stream) {
  return handle_get_state("aog_altmirror_get_state", "mirror", m, blob_dev, stream);
}

int aog_altmirror_set_state(aog_altmirror* m, const void* blob_dev, void* stream) {
  if (int rc = handle_set_state("aog_altmirror_set_state", "mirror", m, blob_dev, stream)) return rc;
  return synthesise(m, record(m), nullptr, stream);   // (every surface from the commands just copied, behind the copy on `stream`)
}

}  // extern "C"
