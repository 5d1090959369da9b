// Host-side helpers shared by the translation units of libaogym.so (not part of the C-ABI).
#pragma once
#include "aogym_internal.h"
#include "k_common.h"   // split_f16, for pack_tab16_rows: the host packs operands with the split the kernels use

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace aog {
struct ActorArgs;
struct ActorNoise;
struct PhaseFieldArgs;
struct DetectorArgs;
}

namespace aog_host {

// sets aog_last_error() of the calling thread and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return ::aog_host::fail(AOG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

using aog::kLdsBytes;

int dev_alloc_bytes(aog_env* e, void** out, size_t bytes, bool zero);
void dev_release_ptr(aog_env* e, void** ptr);
template <typename T>
int dev_alloc(aog_env* e, T** out, size_t count, bool zero = true) {
  void* p = nullptr;
  const int rc = dev_alloc_bytes(e, &p, std::max<size_t>(count, 1) * sizeof(T), zero);
  if (rc == AOG_OK) *out = static_cast<T*>(p);
  return rc;
}
// a buffer made on first use: allocated unless it is there already
template <typename T>
int need(aog_env* e, T** ptr, size_t count, bool zero = false) {
  return *ptr ? AOG_OK : dev_alloc(e, ptr, count, zero);
}
// give a work buffer of the handle back (workspaces that are re-sized when the caller changes the synthesis method or oversampling:
// without this every change would keep the old gigabytes until aog_destroy)
template <typename T>
void dev_release(aog_env* e, T** ptr) {
  void* p = static_cast<void*>(*ptr);
  dev_release_ptr(e, &p);
  *ptr = nullptr;
}

// host table -> a device buffer of the handle: allocate `count` elements at *dst and copy them from src (blocking).  keep: a buffer
// that is already there is written again in place (a table uploaded twice has the same size)
template <typename T>
int upload(aog_env* e, T** dst, const T* src, size_t count, bool keep = false) {
  if (!(keep && *dst))
    if (int rc = dev_alloc(e, dst, count, false)) return rc;
  HIP_TRY(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return AOG_OK;
}
template <typename T>
int upload(aog_env* e, T** dst, const std::vector<T>& src, bool keep = false) {
  return upload(e, dst, src.data(), src.size(), keep);
}

// one launch with `lds` bytes of dynamic LDS on `device`, for handles that are no aog_env: the request for it, the launch and its error check
template <typename... Params, typename... Args>
int launch_with_lds(int device, hipStream_t s, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, const Args&... args) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, device)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}
// an entry point's one launch of a kernel without dynamic LDS on `stream` (void*): makes `device` current, launches, checks — and returns
// from the entry point on failure, with the entry point's own file and line in aog_last_error as HIP_TRY gives them
#define LAUNCH_PLAIN(device, stream, kernel, grid, block, ...)                                      \
  do {                                                                                             \
    HIP_TRY(hipSetDevice(device));                                                                 \
    hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), __VA_ARGS__);     \
    HIP_TRY(hipGetLastError());                                                                    \
  } while (0)

// The records of a handle that is no aog_env (the six of standalone_handle.h, which holds one each): one device buffer, and the
// stream-ordered copies of its checkpoint (*_get_state / *_set_state: `blob` is a device buffer of `bytes` bytes)
struct RecordStore {
  int device = 0;
  size_t bytes = 0;
  char* ptr = nullptr;
  // (the caller has made `dev` current; what the records hold at first is the handle's own business)
  hipError_t alloc(int dev, size_t n) {
    device = dev;
    bytes = n;
    return hipMalloc(reinterpret_cast<void**>(&ptr), n);
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
  }
  int copy(void* dst, const void* src, void* stream) const {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return AOG_OK;
  }
  int copy_out(void* blob, void* stream) const { return copy(blob, ptr, stream); }
  int copy_in(const void* blob, void* stream) const { return copy(ptr, blob, stream); }
};

// zero `n_words` 32-bit words at p on stream s with a kernel of the library (see k_zero_words for why not hipMemsetAsync)
void zero_words(void* p, size_t n_words, hipStream_t s);

// HIP-event bracket around the launches of one kernel id while profiling is on (aog_profile_read_kernel): the closing record is made by
// the destructor, on the same stream.
struct TimedRegion {
  aog_env* e;
  hipStream_t s;
  hipEvent_t ev1 = nullptr;
  TimedRegion(aog_env* env, hipStream_t stream, int kernel_id, bool on = true) : e(env), s(stream) {
    if (!e->profile || !on) return;
    hipEvent_t ev0 = nullptr;
    if (e->events_used == e->events.size()) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      e->events.emplace_back(a, b);
    }
    ev0 = e->events[e->events_used].first;
    ev1 = e->events[e->events_used].second;
    if (e->event_kernel.size() <= e->events_used) e->event_kernel.resize(e->events_used + 1);
    e->event_kernel[e->events_used] = kernel_id;
    ++e->events_used;
    (void)hipEventRecord(ev0, s);
  }
  ~TimedRegion() {
    if (ev1) (void)hipEventRecord(ev1, s);
  }
  TimedRegion(const TimedRegion&) = delete;
  TimedRegion& operator=(const TimedRegion&) = delete;
};

// The handle's status word (bit 0: a bounded inter-workgroup wait of k_extrude16_split timed out, bit 1: a step failed after its counters
// had moved).  It lives in pinned, device-mapped host memory: reading it costs one load and no synchronisation.  Only these three touch it.
int poisoned(const aog_env* e);
void poison(aog_env* e, int bits);
int clear_poison(aog_env* e);   // the host word and the device-side sticky word (the caller has drained the streams that could set them)
int check_poisoned(const aog_env* e, const char* who);
int refuse_pre_evolved(const aog_env* e, const char* who);
// The checks every off-step instrument's call shares, in this order: tables and screens there; the instrument's own tables uploaded
// (`ready`; `what` = "the science camera was", upload_name = "aog_upload_science"); check_poisoned; refuse_pre_evolved
int instrument_gate(const aog_env* e, const char* who, bool ready, const char* what, const char* upload_name);
int clear_poison_if_whole(aog_env* e, int first, int count, hipStream_t s);
// AOG_ERR_INVALID unless envs [first, first + count) lie inside [0, B)
int check_env_range(const char* who, int first, int count, int B);
// metres of optical path -> revolutions of the wavefront sensor's wavelength
inline double rev_per_metre(const aog_env* e) { return 1.0 / (2.0 * M_PI * e->cfg.wavelength_wfs); }
// Event timing samples launch number `phase` of a handle: blocks of profile_block consecutive launches, the MIDDLE block of each period
// of profile_every blocks (a short window's first launches come right after a synchronisation and are its slowest; two event records cost
// ~6 us on the stream, so a throughput measurement that also wants kernel durations does not time every launch)
inline bool profile_sampled(const aog_env* e, unsigned phase) {
  return ((phase / (unsigned)e->profile_block) % (unsigned)e->profile_every) == (unsigned)e->profile_every / 2;
}
int set_screens_f32(aog_env* e, const float* psi, int first, int count, hipStream_t s, bool means_ready = false);   // means_ready: pack_mean[0 .. count) holds the aperture means already   // device screens [count][N][N] -> internal layouts
// act_dm -> the operand layouts of the fused and phase kernels, in buffers of the caller's choosing
struct ActTargets {
  float* act_rev;     // [A_pad][Bp] fp32 (nullable)
  _Float16* act16;    // split-f16 B operands
  _Float16* act_ll;   // nullable third f16 term of the actuators (K4, K11)
};
// (act_src: nullable [B][A] float64 device actuators to load instead of the mirror's)
int load_actuators(aog_env* e, hipStream_t s, ActTargets to, const double* act_src = nullptr);
// focal.hip: the operand prologue of an off-step instrument's call on a fast handle — psi_tile holding the screens the last step read
// (obs_tiles) and the actuators (the mirror's, or act_src) in e->inst_act16 and, with want_ll, e->inst_act_ll, made on first need
int instrument_operands(aog_env* e, hipStream_t s, bool want_ll, const double* act_src = nullptr);
// The kernels instantiated per padded mode count outside the step path: f(std::integral_constant<int, 16 | 32 | 64 | 128>) for A_pad (anything
// else gets 128), e.g. with_apad(e->A_pad, [&](auto apad) { hipLaunchKernelGGL((k<apad()>), ...); }).  (The step path's own table of
// launchers is launchers_for in aogym.hip.)
template <typename F>
void with_apad(int A_pad, F&& f) {
  switch (A_pad) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: f(std::integral_constant<int, 128>{}); break;
  }
}
// The A operand of a contraction over the pixels of a tile with accumulator-order values as its B operand (k_pupil_tile.h), per pixel
// tile and in tab16's pixel order: [pixel tile][block of 32 rows][step 2][hi | lo][lane (kg, row & 31)][el] <-> row `row` at pixel
// (el & 3) + 16 s + 8 (el >> 2) + 4 kg of the tile; value(p, row) x scale is split like modes16.  Pad pixels and pad rows are zeros.
template <typename V>
std::vector<_Float16> pack_tab16_rows(int n_ptiles, int n_ap, int rows, int nblk, float scale, V&& value) {
  std::vector<_Float16> t16((size_t)n_ptiles * nblk * 2 * 2 * 64 * 8, (_Float16)0.f);
  for (int pt = 0; pt < n_ptiles; ++pt)
    for (int sidx = 0; sidx < 2; ++sidx)
      for (int kg = 0; kg < 2; ++kg)
        for (int el = 0; el < 8; ++el) {
          const int p = pt * 32 + (el & 3) + 16 * sidx + 8 * (el >> 2) + 4 * kg;
          if (p >= n_ap) continue;
          for (int k = 0; k < rows; ++k) {
            _Float16 hi, lo;
            aog::split_f16((float)value(p, k) * scale, hi, lo);
            const size_t base = (((((size_t)pt * nblk + (k >> 5)) * 2 + sidx) * 2) * 64 + (kg * 32 + (k & 31))) * 8 + el;
            t16[base] = hi;
            t16[base + (size_t)64 * 8] = lo;
          }
        }
  return t16;
}
// iy << 16 | ix of every aperture pixel, from the host copy of ap_index
std::vector<int32_t> ap_yx_table(const aog_env* e);
// Launchers of the kernels instantiated per padded mode count, one translation unit each so the build parallelises (fused_inst.hip compiled
// with -DAOG_INST_APAD=16|32|64|128 defines apad_launchers<that count>).  Each returns 0 or the aog_status of a failed dynamic-LDS request.
struct ApadLaunchers {
  int (*fused)(aog_env* e, hipStream_t s);
  int (*phase)(aog_env* e, hipStream_t s, const _Float16* act16, float* out_tile);
  int (*phase_field)(aog_env* e, hipStream_t s, const _Float16* act16, const aog::PhaseFieldArgs& fa, bool grid);
  int (*phase_grid)(aog_env* e, hipStream_t s, const _Float16* act16, const aog::PhaseFieldArgs& fa, int etile0, int n_et);
};
template <int A_PAD>
const ApadLaunchers& apad_launchers();
// phase-only contraction u = psi + Mt a for every (pixel, env) with the actuator operands `act16`, written in the psi_tile layout
void launch_phase(aog_env* e, hipStream_t s, const _Float16* act16, float* out_tile);
void launch_phase_grid(aog_env* e, hipStream_t s, const _Float16* act16, const _Float16* act_ll, float* grid, size_t env_stride, int row_stride, int etile0,
                       int n_et);
void launch_phase_field(aog_env* e, hipStream_t s, const _Float16* act16, float* field, size_t env_stride, int row_stride, bool grid);   // complex64 field, or (grid) one float of reduced phase per pixel
// focal.hip (K11): the observation of the separable route for every env — |F|^2 into obs_pw and the caller's obs_raw / obs (nullable)
// (mask: the masked reset's; handles with a detector draw for the masked envs only)
int launch_obs(aog_env* e, hipStream_t s, float* obs_raw, uint16_t* obs, const uint8_t* mask = nullptr);
// focal.hip (K11): pass 1 alone for the first n envs of obs_work — grid -> T16 (the observation gradient runs its own pass 2 behind it)
void launch_obs_pass1(aog_env* e, hipStream_t s, int n);
// the detector's kernel arguments for the observation this call writes (e->det_on): frame = e->obs_frame
aog::DetectorArgs detector_args(const aog_env* e, const uint8_t* mask);
// gradient_obs.hip (K14 on the separable route, after aog_upload_gradient_obs): the observation's part of one aog_output_gradient call, behind
// its k_grad_coef — the float64 obs_raw into the observation slots of `values` (nullable) and, with g_obs (nullable), the modes contraction of
// the observation's q into e->gobs_slabs for k_grad_finish.  The actuator operands (inst_act16, inst_act_ll) are the caller's.
int grad_obs_part(aog_env* e, hipStream_t s, const double* g_obs_dev, double* values_dev);
// pyramid.hip: the checks every call on an uploaded sensor shares (instrument_gate), and the sum over the modulation points of every selected env into pyr_acc
// (no division yet) at the mirror's actuators or at act_src (nullable [B][A] device) — the forward launches of aog_pyramid_frames, which
// aog_pyramid_gradient (pyramid_grad.hip) runs for its clean frame
int pyramid_ready(aog_env* e, const char* who);
int pyramid_accumulate(aog_env* e, hipStream_t s, const uint8_t* mask_dev, const double* act_src = nullptr);
// pyramid.hip, float64 handles: modulation point j of one env — F_j (launch_mft64; the field with j = 0), X = b1 F_j, the quadrants G = X b2
void launch_pyramid_point64(aog_env* e, hipStream_t s, int j, int env, const uint8_t* mask_dev, const double* act_src);
// pyramid.hip, fast handles: the steps of that sum, for the gradient's backward sweep — psi_tile and the call's own actuator operands (and
// psi_tile put back), the phase grid of a chunk's envs into pyr_work.grid, F_j of the chunk into pyr_fop (the two forward passes), and the
// 16-row k-steps of the window's two halves
int pyramid_operands_begin(aog_env* e, hipStream_t s, const double* act_src);
int pyramid_operands_end(aog_env* e, hipStream_t s);
void pyramid_phase_grid(aog_env* e, hipStream_t s, int env0, int n);
void pyramid_forward_point(aog_env* e, hipStream_t s, int j, int env0, int n, const uint8_t* mask_dev);
int4 pyramid_halves(const aog_env* e);
// gradient_obs.hip: k_grad_obs_backward on a q grid [n][grid_env] (row stride Nxp) of n envs from env tile env0 / 32 on, into slabs
// [pupil_chunks][A_pad][Bp] (+ env0 applied here); needs grad_mtab16 (aog_upload_gradient)
void launch_grad_obs_backward(aog_env* e, hipStream_t s, const float* qgrid, size_t grid_env, int Nxp, int env0, int n, double* slabs);
// pyramid_grad.hip: gives the gradient's work buffers back (aog_upload_pyramid: they are sized by the sensor)
void release_pyramid_gradient(aog_env* e);
// screens.hip: the factors through which Cn^2 enters (null outputs are skipped) — the handle-wide value's and every per-env value's
void turbulence_factors(int N, int oversampling, double pixel_pitch, double cn_squared, float* amp_high, float* amp_low, float* crop_scale,
                        double* sqrt_cn_squared);
// per-env sqrt(Cn^2) and int8 noise scales from the handle's per-env values (no-op without them); AOG_ERR_INVALID if one is above the layer's
int turbulence_refresh_f64(aog_env* e, hipStream_t s);
// atmosphere.hip
int pack_from_master(aog_env* e, int first, int count, hipStream_t s, bool per_step = false);
int evolve_layer(aog_env* e, hipStream_t s, long long step_index);
int x8_drop_ahead(aog_env* e);   // before anything the int8 extrusion's work ahead (plan, x phase of the next step) read is changed
int ensure_tiles(aog_env* e, hipStream_t s);
int obs_tiles(aog_env* e, hipStream_t s);   // psi_tile holding the screens this step's fused kernel read (the separable observation route)
int ring_from_master(aog_env* e, int first, int count, int keep_ref, hipStream_t s);
int store_master_f64(aog_env* e, const double* psi, int first, int count, hipStream_t s);
int store_master_f32(aog_env* e, const float* psi, int first, int count, hipStream_t s);
int unroll_master(aog_env* e, double* psi_dev, int first, int count, hipStream_t s);
// actor.hip: the checks and arguments of a policy query (aog_actor_act, aog_step_act): all but the observations and outputs; *lds = the query's
// dynamic LDS (activations + weight chunk).  AOG_ERR_UNSUPPORTED (naming the sizes) when they do not fit.
int actor_args(const aog_actor* net, const char* who, aog::ActorArgs* out, size_t* lds);
// actor.hip: the checks of an aog_action_noise (NULL: none, AOG_OK) and its kernel form; *noisy = the query runs the NOISE instantiation.
int action_noise_args(const aog_action_noise* nz, const char* who, aog::ActorNoise* out, bool* noisy);

}  // namespace aog_host
