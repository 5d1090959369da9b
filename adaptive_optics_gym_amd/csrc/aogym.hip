// libaogym.so — C-ABI (include/aogym.h) over the gfx950 kernels in the k_*.h headers.
// Host side only: argument checking, table conversion/upload, launch geometry, stream-ordered launches.
#include "mft_host.h"
#include "k_pack.h"
#include "k_step.h"
#include "k_step_act.h"
#include "k_step_spgd.h"
#include "spgd_host.h"

#include <hipfft/hipfft.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#ifdef AOG_DEV
namespace aog_host { long long* dev_timeline = nullptr; }
extern "C" int aog_dev_read_timeline(void* dst, size_t nbytes) {   // developer builds only: not in include/aogym.h
  if (!aog_host::dev_timeline) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpy(dst, aog_host::dev_timeline, nbytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

namespace aog_host {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int ensure_dynamic_lds(const void* fn, size_t bytes, int device) {
  if (bytes <= 64 * 1024) return AOG_OK;   // the default limit
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> granted;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[{fn, device}];
  if (bytes > have) {
    const hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) {
      (void)hipGetLastError();   // (a refused request is reported here; it must not surface again at the next unrelated error check)
      return fail(AOG_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu bytes) failed: %s", bytes, hipGetErrorString(err));
    }
    have = bytes;
  }
  return AOG_OK;
}

int dev_alloc_bytes(aog_env* e, void** out, size_t bytes, bool zero) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  if (zero) {
    // the fill runs on the null stream, which a non-blocking caller's stream does not wait for, and hipMemset on device memory may return
    // before it has run: wait for it here, so that whatever stream reads the buffer first finds the zeros (an allocation path only)
    HIP_TRY(hipMemset(p, 0, bytes));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  e->allocs.push_back(p);
  e->alloc_bytes.push_back(bytes);
  e->dev_bytes += (int64_t)bytes;
  *out = p;
  return AOG_OK;
}

// give a work buffer of the handle back (workspaces that are re-sized when the caller changes the synthesis method or oversampling:
// without this every change would keep the old gigabytes until aog_destroy)
void dev_release_ptr(aog_env* e, void** ptr) {
  if (!*ptr) return;
  for (size_t i = 0; i < e->allocs.size(); ++i)
    if (e->allocs[i] == *ptr) {
      e->dev_bytes -= (int64_t)e->alloc_bytes[i];   // (aog_info.device_bytes stays what the handle owns)
      e->allocs.erase(e->allocs.begin() + (long)i);
      e->alloc_bytes.erase(e->alloc_bytes.begin() + (long)i);
      break;
    }
  (void)hipFree(*ptr);
  *ptr = nullptr;
}

// zero `n_words` 32-bit words at p on stream s with a kernel of the library (see k_zero_words for why not hipMemsetAsync)
void zero_words(void* p, size_t n_words, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<size_t>((n_words + 255) / 256, 4096);
  if (n_words) hipLaunchKernelGGL(aog::k_zero_words, dim3(blocks), dim3(256), 0, s, static_cast<uint32_t*>(p), n_words);
}

int poisoned(const aog_env* e) { return e->host_flag ? *static_cast<volatile const int*>(e->host_flag) : 0; }

void poison(aog_env* e, int bits) {
  if (e->host_flag) *static_cast<volatile int*>(e->host_flag) |= bits;
}

int clear_poison(aog_env* e) {
  HIP_TRY(hipMemset(e->dev_status, 0, sizeof(int)));
  *static_cast<volatile int*>(e->host_flag) = 0;
  e->reset_obs_valid = false;   // (whatever the failed call left behind, the next reset observes it afresh)
  return AOG_OK;
}

// A bounded inter-workgroup wait of an earlier launch timed out (k_extrude16_split): every screen that launch touched is suspect.
// The status word is seen at the latest by the call after the one whose launch tripped it.  Installing fresh screens for the whole batch
// (aog_set_screens / aog_set_state) clears it.
int check_poisoned(const aog_env* e, const char* who) {
  if (const int bits = poisoned(e))
    return fail(AOG_ERR_STATE, "%s: %s; the screens of this handle are invalid (install new screens for the whole batch or restore a saved state)", who,
                (bits & 2) ? "an earlier aog_step failed after its counters had moved"
                           : "an inter-workgroup wait of the dynamic-atmosphere kernel timed out in an earlier step");
  return AOG_OK;
}

// With lookahead on, between aog_step(t) and aog_step(t + 1) the screens already stand at step t + 1: anything that reads or replaces
// them then would see (or break) a state the env is not in.  Episode boundaries are safe: the last step of an episode does not look ahead.
int refuse_pre_evolved(const aog_env* e, const char* who) {
  if (e->pro_pending)
    return fail(AOG_ERR_STATE, "%s: a pipelined step has already loaded the NEXT action into the mirror (aog_step_pipelined with action_next): finish "
                "the sequence with action_next = NULL (or reset the whole batch) first", who);
  if (e->pre_evolved)
    return fail(AOG_ERR_STATE, "%s: the atmosphere of this handle has been advanced to the next step already (aog_set_lookahead): call it at an "
                "episode boundary (after a step that returned done), or switch lookahead off and take one more step first", who);
  return AOG_OK;
}

int instrument_gate(const aog_env* e, const char* who, bool ready, const char* what, const char* upload_name) {
  if (!e->tables_ready || !e->screens_ready) return fail(AOG_ERR_STATE, "%s before aog_upload_tables/aog_set_screens", who);
  if (!ready) return fail(AOG_ERR_STATE, "%s: %s not uploaded (%s, again after aog_upload_tables)", who, what, upload_name);
  if (int rc = check_poisoned(e, who)) return rc;
  return refuse_pre_evolved(e, who);
}

int check_env_range(const char* who, int first, int count, int B) {
  if (first < 0 || count < 0 || first + count > B) return fail(AOG_ERR_INVALID, "%s: env range [%d,%d) outside [0,%d)", who, first, first + count, B);
  return AOG_OK;
}

int load_actuators(aog_env* e, hipStream_t s, ActTargets to, const double* act_src) {
  const int n = e->B * e->A_pad;
  hipLaunchKernelGGL(aog::k_load_actuators, dim3((n + 255) / 256), dim3(256), 0, s, act_src ? act_src : e->act_dm, to.act_rev, to.act16, e->B, e->A, e->A_pad,
                     e->Bp, 2.0 / e->cfg.wavelength_wfs, to.act_ll);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

std::vector<int32_t> ap_yx_table(const aog_env* e) {
  const int N = e->cfg.n_pupil;
  std::vector<int32_t> yx(e->ap_index_host.size());
  for (size_t i = 0; i < yx.size(); ++i) yx[i] = ((e->ap_index_host[i] / N) << 16) | (e->ap_index_host[i] % N);
  return yx;
}

// New screens for the WHOLE batch make a handle whose extrusion kernel once timed out usable again (see check_poisoned).  Called by the
// public entry points with the range of the whole call (aog_generate_screens installs large batches in several chunks).  Dynamic handles
// drain the stream first: a timeout of a launch that is still running would otherwise poison the screens just installed.
int clear_poison_if_whole(aog_env* e, int first, int count, hipStream_t s) {
  if (first != 0 || count != e->B) return AOG_OK;
  if (e->cfg.atm_dynamic) HIP_TRY(hipStreamSynchronize(s));
  if (poisoned(e)) {
    HIP_TRY(hipStreamSynchronize(s));
    return clear_poison(e);
  }
  return AOG_OK;
}

// "anything else takes the 128 launchers": float64 validation handles (A_pad a multiple of 8) never launch through them
const ApadLaunchers& launchers_for(int A_pad) {
  switch (A_pad) {
    case 16: return apad_launchers<16>();
    case 32: return apad_launchers<32>();
    case 64: return apad_launchers<64>();
    default: return apad_launchers<128>();
  }
}

// grid = true: one float per pixel (reduced phase) instead of the complex field: see k_phase_mfma<.., GRID>
void launch_phase_field(aog_env* e, hipStream_t s, const _Float16* act16, float* field, size_t env_stride, int row_stride, bool grid) {
  aog::PhaseFieldArgs fa{};
  fa.ap_yx = e->sh_ap_yx;
  fa.mla32 = reinterpret_cast<const float2*>(e->sh_mla32);
  fa.mla_rev = e->sh_ftab;
  fa.field = reinterpret_cast<float2*>(field);
  fa.env_stride = env_stride;
  fa.row_stride = row_stride;
  fa.n_ap = e->n_ap;
  fa.B = e->B;
  fa.N = e->cfg.n_pupil;
  fa.amplitude = (float)e->sh_amp;
  launchers_for(e->A_pad).phase_field(e, s, act16, fa, grid);
}
void launch_phase_grid(aog_env* e, hipStream_t s, const _Float16* act16, const _Float16* act_ll, float* grid, size_t env_stride, int row_stride, int etile0,
                       int n_et) {
  aog::PhaseFieldArgs fa{};
  fa.ap_yx = e->focal_ap_yx;
  fa.mla_rev = nullptr;
  fa.act_ll = reinterpret_cast<const aog::f16x8*>(act_ll) + (size_t)etile0 * (e->A_pad / 16) * 64;
  fa.field = reinterpret_cast<float2*>(grid);   // grid row 0 = env etile0 * 32
  fa.env_stride = env_stride;
  fa.row_stride = row_stride;
  fa.n_ap = e->n_ap;
  fa.B = e->B - etile0 * 32;
  fa.N = e->cfg.n_pupil;
  launchers_for(e->A_pad).phase_grid(e, s, act16, fa, etile0, n_et);
}
void launch_phase(aog_env* e, hipStream_t s, const _Float16* act16, float* out_tile) { launchers_for(e->A_pad).phase(e, s, act16, out_tile); }

aog::DetectorArgs detector_args(const aog_env* e, const uint8_t* mask) {
  aog::DetectorArgs d{};
  d.par = e->det_par;
  d.mask = mask;
  d.seed = e->rng_seed;
  d.frame_lo = (uint32_t)e->obs_frame;
  d.frame_hi = (uint32_t)(e->obs_frame >> 32);
  d.env_base = e->cfg.env_id_base;
  d.B = e->B;
  return d;
}
}  // namespace aog_host
using namespace aog_host;

namespace {

int pick_pad(int v, const int* opts, int n) {
  for (int i = 0; i < n; ++i)
    if (v <= opts[i]) return opts[i];
  return -1;
}

const int kApadOpts[] = {16, 32, 64, 128};
const int kMrwOpts[] = {7, 12, 20, 28};

const char kFastSizesMsg[] = "%s: fast kernels are built for act_dim <= 128, <= 28 wfs tables and 1 science table; use AOG_PRECISION_FP64 for this shape";

// The fast kernels' padded sizes and the fused pass's launch geometry for a shape: the one place aog_create and aog_fused_plan take them from.
struct FusedPlan {
  int Bp, n_ap_pad, A_pad, MRW;
  aog::FusedGeom geom;
};
int plan_fused(const char* who, int num_envs, int n_ap, int n_modes, int n_wfs_tables, bool mfma, bool atm_dynamic, int pixel_chunks, bool four_wave,
               FusedPlan* p) {
  p->Bp = round_up(num_envs, 64);
  p->n_ap_pad = round_up(n_ap, 32);
  p->A_pad = pick_pad(n_modes, kApadOpts, 4);
  p->MRW = pick_pad(n_wfs_tables, kMrwOpts, 4);
  if (p->A_pad < 0 || p->MRW < 0)
    return fail(AOG_ERR_UNSUPPORTED, kFastSizesMsg, who);
  p->geom = aog::fused_geometry(p->Bp, p->n_ap_pad, p->A_pad, p->MRW, mfma, atm_dynamic, pixel_chunks, four_wave);
  if (mfma && !aog::fused_geometry_fits(p->geom, p->A_pad, p->MRW, atm_dynamic))
    return fail(AOG_ERR_UNSUPPORTED,
                "%s: the fused pupil pass has no launch form for B=%d n_ap=%d act_dim=%d with %d wfs tables, %s atmosphere: %d waves and %d pixel tiles "
                "per chunk need %d bytes of LDS (> %zu)",
                who, num_envs, n_ap, n_modes, n_wfs_tables, atm_dynamic ? "dynamic" : "static", p->geom.waves, p->geom.tpc,
                aog::FusedLds(p->geom.tpc, p->geom.waves, p->A_pad, p->MRW, atm_dynamic).total, aog_host::kLdsBytes);
  return AOG_OK;
}

int launch_fused(aog_env* e, hipStream_t s) {
  const bool timed = e->profile && profile_sampled(e, e->profile_phase++);   // (this launch advances the counter: evolve_layer only reads it)
  TimedRegion tr(e, s, AOG_PROF_FUSED, timed);
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    hipLaunchKernelGGL(aog::k_fused_ref, dim3(e->B), dim3(256), 0, s, e->modes64, e->tabs64, e->psi64, e->act_dm,
                       e->partials, e->n_ap, e->A, e->MRW_used, e->MRS_used, e->Bp, e->cfg.wavelength_wfs,
                       e->cfg.wavelength_sci);
  } else if (int rc = launchers_for(e->A_pad).fused(e, s)) {
    return rc;   // (the dynamic-LDS request of this shape was refused: the message names the size)
  }
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

// The epilogue's dynamic LDS.  e->MRW / e->MRS are the table counts the partial slabs hold: the padded counts of the fast kernels, and the
// counts in use on float64 validation handles (aog_create sets them so), whose single slab k_fused_ref writes.
// Handles with a detector add the plane of noisy observations (table route: n_obs_tab x 16 doubles).
size_t epilogue_lds(const aog_env* e, bool detector) {
  return aog::EpilogueLds(e->MRW, e->MRS, e->n_out, e->MRW_used, e->MRS_used, detector ? e->n_obs_tab : 0).bytes();
}
size_t epilogue_lds(const aog_env* e) { return epilogue_lds(e, e->det_on); }

// the policy attached to aog_reset_act / aog_step_act: its arguments (actor_args, checked before the call changes anything) and outputs
struct ActTail {
  aog::ActorArgs a;
  size_t lds = 0;      // the query's own dynamic LDS
  aog::ActorNoise nz{};
  bool noisy = false;  // nz needs k_epilogue_act_prologue_noise (aog_action_noise: mean mode / OU term)
  bool spgd = false;   // aog_reset_spgd / aog_step_spgd: the SPGD query `sp` rides in the policy's place (k_epilogue_spgd_prologue), `a` is unused
  aog::SpgdArgs sp{};
};

// the prologue of a step from `action` (k_prologue, k_epilogue_prologue, k_epilogue_act_prologue)
aog::PrologueArgs prologue_args(const aog_env* e, const float* action) {
  aog::PrologueArgs q{};
  // each fused kernel reads one operand layout: write only that one (the float64 device kernel and the VALU kernel read act_rev)
  const bool mfma_fast = e->kernel == AOG_KERNEL_MFMA && e->cfg.precision == AOG_PRECISION_FAST && !e->sh_ready;
  q.action = action;
  q.gram = e->gram;
  q.act_dm = e->act_dm;
  q.act_rev = mfma_fast ? nullptr : e->act_rev;
  q.act16 = e->act16;
  q.B = e->B; q.A = e->A; q.A_pad = e->A_pad; q.Bp = e->Bp;
  q.sh_operation = e->cfg.sh_operation;
  q.target = e->cfg.surface_rms_target;
  q.two_over_lambda = 2.0 / e->cfg.wavelength_wfs;
  return q;
}

// the epilogue's arguments for one reset (is_step = false: the step outputs are null) or step, writing into the caller's tensors
aog::EpilogueArgs epilogue_args(const aog_env* e, bool is_step, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done, float* power,
                                float* strehl) {
  aog::EpilogueArgs p{};
  p.partials = e->partials;
  p.wfs_coef = e->wfs_coef;
  p.sci_coef = e->sci_coef;
  p.obs_raw = obs_raw;
  p.obs = obs;
  p.reward = reward;
  p.done = done;
  p.power = power;
  p.strehl = strehl;
  p.t_render = e->t_render;
  p.B = e->B;
  p.Bp = e->Bp;
  p.n_chunks = e->geom.n_chunks;
  p.MRW = e->MRW;   // (see epilogue_lds)
  p.MRS = e->MRS;
  p.MRW_used = e->MRW_used;
  p.MRS_used = e->MRS_used;
  p.n_obs = e->n_obs_tab;
  p.obs_pw = e->obs_sep ? e->obs_pw : nullptr;
  p.n_obs_sep = e->obs_sep ? e->n_obs : 0;
  p.n_fiber = e->cfg.n_fiber_modes;
  p.reward_type = e->cfg.reward_type;
  p.has_thr = e->cfg.has_rew_threshold;
  p.max_steps = e->cfg.max_steps;
  p.is_step = is_step ? 1 : 0;
  p.ret_acc = is_step ? e->ret_acc : nullptr;
  p.thr = e->cfg.rew_threshold;
  p.ssim_peak = e->cfg.ssim_ref_peak;
  p.ssim_alpha = e->cfg.ssim_alpha;
  return p;
}

// one launch with `lds` bytes of dynamic LDS: the request for it, the launch and its error check
template <typename... Params, typename... Args>
int launch_with_lds(const aog_env* e, hipStream_t s, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, const Args&... args) {
  if (int rc = aog_host::ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, e->device)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

// The last launch of a reset or step, in one of three forms that are worked out once:
//   plain                                     k_epilogue               n_epi workgroups of 1024, the epilogue's LDS
//   action_next (aog_step_pipelined)          k_epilogue_prologue      the prologue of the NEXT step rides in the same launch, in workgroups of
//                                                                      its own behind the epilogue's
//   tail (aog_reset_act / aog_step_act)       k_epilogue_act_prologue  the policy query on this epilogue's observation and the prologue of the next
//                                             (_noise: tail->noisy)    step from its action ride in the same launch, per workgroup of 16 envs
//   tail->spgd (aog_reset_spgd / aog_step_spgd) k_epilogue_spgd_prologue the same with the SPGD query on this epilogue's metric in the policy's place
// Handles with a detector (e->det_on) launch the same form through the _det kernel of that name, which draws the detector's noise: the same
// grid, block and arguments, its LDS from epilogue_lds, and DetectorArgs appended.
// mask (masked aog_reset): handles with a detector draw for the masked envs only
int launch_epilogue(aog_env* e, bool is_step, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done, float* power,
                    float* strehl, hipStream_t s, const float* action_next = nullptr, const ActTail* tail = nullptr, const uint8_t* mask = nullptr) {
  const aog::EpilogueArgs p = epilogue_args(e, is_step, obs_raw, obs, reward, done, power, strehl);
  const size_t lds = epilogue_lds(e);
  const int n_epi = (e->Bp + aog::kEpiEnvs - 1) / aog::kEpiEnvs;
  const auto launch = [&](auto* plain, auto* det, dim3 grid, dim3 block, size_t bytes, const auto&... args) {
    return e->det_on ? launch_with_lds(e, s, det, grid, block, bytes, p, args..., detector_args(e, mask))
                     : launch_with_lds(e, s, plain, grid, block, bytes, p, args...);
  };
  if (tail && tail->spgd)
    return launch(aog::k_epilogue_spgd_prologue, aog::k_epilogue_spgd_prologue_det, dim3(n_epi), dim3(aog::kStepSpgdThreads),
                  aog::step_spgd_lds_bytes(lds), tail->sp, prologue_args(e, tail->sp.action));
  if (tail) {
    aog::ActorArgs a = tail->a;
    a.obs = obs;
    a.obs_f16 = 1;
    const aog::PrologueArgs q = prologue_args(e, a.action);
    const int obs_from_lds = e->obs_sep ? 0 : 1;
    const dim3 grid(n_epi), block(aog::kStepActThreads);
    const size_t lds_all = aog::step_act_lds_bytes(lds, tail->lds);   // (<= kLdsBytes: checked by step_act_tail)
    if (tail->noisy)
      return launch(aog::k_epilogue_act_prologue_noise, aog::k_epilogue_act_prologue_noise_det, grid, block, lds_all,
                    aog::ActorNoiseArgs{a, tail->nz}, q, obs_from_lds);
    return launch(aog::k_epilogue_act_prologue, aog::k_epilogue_act_prologue_det, grid, block, lds_all, a, q, obs_from_lds);
  }
  if (action_next)
    return launch(aog::k_epilogue_prologue, aog::k_epilogue_prologue_det, dim3(n_epi + (e->B + aog::kEpiProEnvs - 1) / aog::kEpiProEnvs), dim3(1024), lds,
                  prologue_args(e, action_next), n_epi);
  return launch(aog::k_epilogue, aog::k_epilogue_det, dim3(n_epi), dim3(1024), lds);
}

template <typename T>
int set_screens(aog_env* e, const T* psi, int first, int count, hipStream_t s, bool means_ready = false) {
  if (!e || !psi) return fail(AOG_ERR_INVALID, "aog_set_screens: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_set_screens before aog_upload_tables");
  if (int rc = check_env_range("aog_set_screens", first, count, e->B)) return rc;
  if (int rc = refuse_pre_evolved(e, "aog_set_screens")) return rc;
  if (int rcd = x8_drop_ahead(e)) return rcd;   // (work done ahead for the next step read the state this call changes)
  if (count == 0) return AOG_OK;
  e->reset_obs_valid = false;   // new screens for any env: the cached reset observation is of the old ones
  HIP_TRY(hipSetDevice(e->device));
  const double inv = rev_per_metre(e);
  const int N2 = e->cfg.n_pupil * e->cfg.n_pupil;
  if (e->cfg.atm_dynamic) {
    if (int rcs = std::is_same<T, double>::value ? store_master_f64(e, reinterpret_cast<const double*>(psi), first, count, s)
                                                 : store_master_f32(e, reinterpret_cast<const float*>(psi), first, count, s))
      return rcs;
    int rc = e->ring_direct ? ring_from_master(e, first, count, 0, s) : pack_from_master(e, first, count, s);
    if (rc != AOG_OK) return rc;
  } else if (e->cfg.precision == AOG_PRECISION_FAST && count >= 8) {
    // batches: aperture means, then tiled conversion with whole-line stores (k_pack_tiles)
    if (!e->pack_mean) {
      int rc = dev_alloc(e, &e->pack_mean, (size_t)e->B, false);
      if (rc != AOG_OK) return rc;
    }
    TimedRegion tr(e, s, AOG_PROF_PACK);
    // (means_ready: the synthesis' last pass summed the aperture while it had the screens in registers: pack_mean[0 .. count) is there)
    if (!means_ready) hipLaunchKernelGGL((aog::k_screen_means<T>), dim3(count), dim3(256), 0, s, psi, e->ap_index, e->pack_mean, N2, e->n_ap);
    const int et0 = first >> 5, et1 = (first + count - 1) >> 5;
    hipLaunchKernelGGL((aog::k_pack_tiles<T>), dim3((e->n_ptiles + aog::kPackTiles - 1) / aog::kPackTiles, et1 - et0 + 1), dim3(256), 0, s, psi,
                       e->ap_index, e->pack_mean, e->psi_rev, e->psi_tile, first, count, N2, e->n_ap, e->n_ptiles, e->Bp, inv);
    HIP_TRY(hipGetLastError());
  } else {
    TimedRegion tr(e, s, AOG_PROF_PACK);
    hipLaunchKernelGGL((aog::k_pack_screens<T>), dim3(count), dim3(256), 0, s, psi, e->ap_index, e->psi_rev, e->psi_tile,
                       e->psi64, first, N2, e->n_ap, e->n_ap_pad, e->Bp, inv, (const int32_t*)nullptr, e->cfg.n_pupil);
    HIP_TRY(hipGetLastError());
  }
  e->screens_ready = true;
  e->sh_sums_ready = false;   // lenslet sums of an earlier aog_sh_image(NULL) belong to the old screens
  return AOG_OK;
}

}  // namespace

namespace aog_host {
int set_screens_f32(aog_env* e, const float* psi, int first, int count, hipStream_t s, bool means_ready) { return set_screens<float>(e, psi, first, count, s, means_ready); }
}  // namespace aog_host

extern "C" {

int aog_abi_version(void) { return AOG_ABI_VERSION; }

#ifndef AOG_BUILD_ID
#define AOG_BUILD_ID "unidentified"
#endif
// (the marker lets build.py read the id out of the file without loading it)
static const char kBuildIdMarker[] = "AOG_BUILD_ID=" AOG_BUILD_ID;
const char* aog_build_id(void) { return kBuildIdMarker + 13; }

const char* aog_last_error(void) { return g_last_error.c_str(); }

int64_t aog_struct_size(int which) {
  switch (which) {
    case 0: return (int64_t)sizeof(aog_config);
    case 1: return (int64_t)sizeof(aog_tables);
    case 2: return (int64_t)sizeof(aog_layer_tables);
    case 3: return (int64_t)sizeof(aog_sh_tables);
    case 4: return (int64_t)sizeof(aog_actor);
    case 5: return (int64_t)sizeof(aog_info);
    case 6: return (int64_t)sizeof(aog_layer_composite);
    case 7: return (int64_t)sizeof(aog_obs_mft);
    case 8: return (int64_t)sizeof(aog_action_noise);
    default: return -1;
  }
}

int aog_create(const aog_config* cfg, int device, aog_env** out) {
  if (!cfg || !out) return fail(AOG_ERR_INVALID, "aog_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != AOG_ABI_VERSION)
    return fail(AOG_ERR_INVALID, "aog_create: abi_version %d != %d", cfg->abi_version, AOG_ABI_VERSION);
  if (cfg->num_envs < 1 || cfg->n_pupil < 2 || cfg->n_modes < 1 || cfg->obs_dim < 1 || cfg->n_ap < 1 ||
      cfg->n_ap > cfg->n_pupil * cfg->n_pupil)
    return fail(AOG_ERR_INVALID, "aog_create: bad sizes (B=%d N=%d A=%d o=%d n_ap=%d)", cfg->num_envs, cfg->n_pupil,
                cfg->n_modes, cfg->obs_dim, cfg->n_ap);
  if (cfg->n_wfs_tables < 1 || cfg->n_sci_tables < 1 || cfg->n_fiber_modes < 0)
    return fail(AOG_ERR_INVALID, "aog_create: bad table counts");
  if (cfg->reward_type != AOG_REWARD_STREHL && cfg->reward_type != AOG_REWARD_SMF_SSIM)
    return fail(AOG_ERR_INVALID, "aog_create: reward_type must be 'strehl_ratio' or 'smf_ssim' (AO_env.py:476,487)");
  if (cfg->obs_separable != 0 && cfg->obs_separable != 1) return fail(AOG_ERR_INVALID, "aog_create: obs_separable must be 0 or 1");
  if (cfg->obs_dim > 32)
    return fail(AOG_ERR_UNSUPPORTED, "aog_create: obs_dim %d > 32 not built (limit 32: the policy kernel aog_actor_act takes state_dim <= 1024 = 32^2)",
                cfg->obs_dim);
  if (!cfg->obs_separable && cfg->obs_dim * cfg->obs_dim > 64)
    return fail(AOG_ERR_UNSUPPORTED, "aog_create: obs_dim > 8 not built on the table route (cfg.obs_separable = 1 takes obs_dim <= 32)");
  if (cfg->n_modes > 256) return fail(AOG_ERR_UNSUPPORTED, "aog_create: act_dim > 256 not built");
  if (cfg->n_wfs_tables + cfg->n_sci_tables > 80) return fail(AOG_ERR_UNSUPPORTED, "aog_create: > 80 tables");
  if (cfg->env_id_base < 0) return fail(AOG_ERR_INVALID, "aog_create: env_id_base must be >= 0");
  if (cfg->precision == AOG_PRECISION_FP64 && !cfg->obs_separable) {
    // the epilogue holds the coefficient matrix of every table output in LDS: at o = 8 (67 wfs tables) that is more than a CU has
    const int n_obs = cfg->obs_dim * cfg->obs_dim;
    const size_t lds = aog::EpilogueLds(cfg->n_wfs_tables, cfg->n_sci_tables, n_obs + cfg->n_fiber_modes, cfg->n_wfs_tables, cfg->n_sci_tables).bytes();
    if (lds > aog_host::kLdsBytes)
      return fail(AOG_ERR_UNSUPPORTED, "aog_create: the table route's epilogue at obs_dim %d needs %zu bytes of LDS (> %zu); use cfg.obs_separable = 1",
                  cfg->obs_dim, lds, aog_host::kLdsBytes);
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(AOG_ERR_HIP, "aog_create: device %d not present (%d HIP devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));

  aog_env* e = new aog_env();
  e->cfg = *cfg;
  e->device = device;
  e->B = cfg->num_envs;
  e->Bp = round_up(e->B, 64);
  e->A = cfg->n_modes;
  e->n_ap = cfg->n_ap;
  e->n_ap_pad = round_up(e->n_ap, 32);
  e->n_quads = e->n_ap_pad / 4;
  e->n_ptiles = e->n_ap_pad / 32;
  e->n_etiles = e->Bp / 32;
  e->MRW_used = cfg->n_wfs_tables;
  e->MRS_used = cfg->n_sci_tables;
  e->n_obs = cfg->obs_dim * cfg->obs_dim;
  e->obs_sep = cfg->obs_separable != 0;
  e->n_obs_tab = e->obs_sep ? 0 : e->n_obs;
  e->n_out = e->n_obs_tab + cfg->n_fiber_modes;
  // sin/cos flavour of the fast kernels: "hwraw" (default; v_sin_f32/v_cos_f32 on the revolutions, the instruction
  // reduces them itself), "hw" (same instructions after an explicit exact reduction), "poly" (degree-7/8 polynomial)
  e->sincos_hw = 2;
  if (const char* sc = getenv("AOG_SINCOS")) e->sincos_hw = strcmp(sc, "poly") == 0 ? 0 : (strcmp(sc, "hwraw") == 0 ? 2 : 1);
  if (const char* v = getenv("AOG_RESET_CACHE")) e->reset_cache = strcmp(v, "0") != 0;

  if (cfg->precision == AOG_PRECISION_FAST) {
    e->MRS = 1;
    e->kernel = cfg->kernel == AOG_KERNEL_AUTO ? AOG_KERNEL_MFMA : cfg->kernel;
    FusedPlan plan;
    int prc = plan_fused("aog_create", e->B, e->n_ap, e->A, e->MRW_used, e->kernel == AOG_KERNEL_MFMA, cfg->atm_dynamic != 0, cfg->pixel_chunks,
                         getenv("AOG_FUSED_4WAVE") != nullptr, &plan);
    if (prc == AOG_OK && e->MRS_used != 1) prc = fail(AOG_ERR_UNSUPPORTED, kFastSizesMsg, "aog_create");
    if (prc != AOG_OK) {
      delete e;
      return prc;
    }
    e->A_pad = plan.A_pad;
    e->MRW = plan.MRW;
    e->geom = plan.geom;
  } else {
    e->A_pad = round_up(e->A, 8);
    e->MRW = e->MRW_used;
    e->MRS = e->MRS_used;
    e->kernel = 0;
    e->geom.n_chunks = 1;
  }

  int rc = AOG_OK;
  const size_t NS = 2 * (size_t)(e->MRW + e->MRS);
  e->partial_elems = (size_t)e->geom.n_chunks * NS * e->Bp;
#define TRY_ALLOC(x) if ((rc = (x)) != AOG_OK) { aog_destroy(e); return rc; }
  TRY_ALLOC(dev_alloc(e, &e->ap_index, e->n_ap));
  TRY_ALLOC(dev_alloc(e, &e->gram, (size_t)e->A * e->A));
  TRY_ALLOC(dev_alloc(e, &e->wfs_coef, (size_t)e->n_out * e->MRW_used * 2));
  TRY_ALLOC(dev_alloc(e, &e->sci_coef, (size_t)e->MRS_used * 2));
  TRY_ALLOC(dev_alloc(e, &e->act_dm, (size_t)e->B * e->A));
  TRY_ALLOC(dev_alloc(e, &e->act_rev, (size_t)e->A_pad * e->Bp));
  TRY_ALLOC(dev_alloc(e, &e->act16, (size_t)e->n_etiles * e->A_pad * 32 * 2));
  TRY_ALLOC(dev_alloc(e, &e->t_render, e->B));
  TRY_ALLOC(dev_alloc(e, &e->screen_gen, e->B));
  TRY_ALLOC(dev_alloc(e, &e->dev_status, 16 + 4 * 2048));   // (16 status words; the rest: developer read-outs)
  {
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      aog_destroy(e);
      return fail(AOG_ERR_HIP, "aog_create: pinned status word allocation failed");
    }
    memset(hp, 0, 64);
    e->host_flag = static_cast<int*>(hp);
    e->host_flag_dev = static_cast<int*>(dp);
  }
  TRY_ALLOC(dev_alloc(e, &e->partials, e->partial_elems));
  if (cfg->atm_dynamic) {
    const size_t N2 = (size_t)cfg->n_pupil * cfg->n_pupil;
    TRY_ALLOC(dev_alloc(e, &e->psi_master, (size_t)e->B * N2));
    TRY_ALLOC(dev_alloc(e, &e->origin, (size_t)e->B * 2));
    e->n_ext_groups = (e->B + aog::kExt16G - 1) / aog::kExt16G;
    TRY_ALLOC(dev_alloc(e, &e->ext_bar, (size_t)2 * round_up(e->n_ext_groups, 8)));   // two ticket sets (see evolve_layer)
    std::vector<int32_t> ident((size_t)e->n_ext_groups * aog::kExt16G, -1);
    for (int i = 0; i < e->B; ++i) ident[i] = i;
    TRY_ALLOC(upload(e, &e->ext_perm, ident));
    TRY_ALLOC(dev_alloc(e, &e->ext_counter, (size_t)e->B));
    TRY_ALLOC(dev_alloc(e, &e->velocity, (size_t)e->B * 2));
    TRY_ALLOC(dev_alloc(e, &e->psi_offset, (size_t)e->B));
    TRY_ALLOC(dev_alloc(e, &e->psi_sum, (size_t)e->B));
  }
  if (cfg->precision == AOG_PRECISION_FAST) {
    const int TROW = round_up(e->MRW + e->MRS, 4);
    TRY_ALLOC(dev_alloc(e, &e->modes_f32, (size_t)e->n_ap_pad * e->A_pad));
    TRY_ALLOC(dev_alloc(e, &e->modes16, (size_t)e->n_ap_pad * e->A_pad * 2));
    TRY_ALLOC(dev_alloc(e, &e->tabs_f32, (size_t)e->n_ap_pad * TROW));
    TRY_ALLOC(dev_alloc(e, &e->tab16, (size_t)e->n_ptiles * 2 * 2 * 64 * 8));
    TRY_ALLOC(dev_alloc(e, &e->sci_tile, (size_t)e->n_ptiles * 32));
    if (e->kernel == AOG_KERNEL_VALU) TRY_ALLOC(dev_alloc(e, &e->psi_rev, (size_t)e->n_quads * e->Bp * 4));   // only the VALU kernel reads this layout
    TRY_ALLOC(dev_alloc(e, &e->psi_tile, (size_t)e->n_etiles * e->n_ptiles * 1024));
  } else {
    TRY_ALLOC(dev_alloc(e, &e->modes64, (size_t)e->n_ap * e->A));
    TRY_ALLOC(dev_alloc(e, &e->tabs64, (size_t)e->n_ap * (e->MRW_used + e->MRS_used)));
    TRY_ALLOC(dev_alloc(e, &e->psi64, (size_t)e->B * e->n_ap));
  }
#undef TRY_ALLOC
  *out = e;
  return AOG_OK;
}

int aog_fused_plan(int num_envs, int n_ap, int n_modes, int n_wfs_tables, int atm_dynamic, int pixel_chunks, int four_wave, int32_t* out) {
  if (!out || num_envs < 1 || n_ap < 1 || n_modes < 1 || n_wfs_tables < 1 || pixel_chunks < 0) return fail(AOG_ERR_INVALID, "aog_fused_plan: bad argument");
  FusedPlan p;
  if (int rc = plan_fused("aog_fused_plan", num_envs, n_ap, n_modes, n_wfs_tables, true, atm_dynamic != 0, pixel_chunks, four_wave != 0, &p)) return rc;
  const aog::FusedGeom& g = p.geom;
  const int32_t v[AOG_FUSED_PLAN_FIELDS] = {
      g.we, g.waves, g.heavy, g.wg_y, g.pair, g.chunks_x, g.tpc, g.n_chunks, p.n_ap_pad / 32, p.Bp / 32, p.A_pad, p.MRW,
      aog::FusedLds(g.tpc, g.waves, p.A_pad, p.MRW, false).total, aog::FusedLds(g.tpc, g.waves, p.A_pad, p.MRW, atm_dynamic != 0).total,
      g.valu_qpc, g.valu_chunks};
  memcpy(out, v, sizeof v);
  return AOG_OK;
}

void aog_destroy(aog_env* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->host_flag) (void)hipHostFree(e->host_flag);
  if (e->turb_ev64) (void)hipEventSynchronize(e->turb_ev64);
  if (e->turb_ev32) (void)hipEventSynchronize(e->turb_ev32);
  if (e->turb_stage64) (void)hipHostFree(e->turb_stage64);
  if (e->turb_stage32) (void)hipHostFree(e->turb_stage32);
  if (e->turb_ev64) (void)hipEventDestroy(e->turb_ev64);
  if (e->turb_ev32) (void)hipEventDestroy(e->turb_ev32);
  if (e->det_ev) (void)hipEventSynchronize(e->det_ev);
  if (e->det_stage) (void)hipHostFree(e->det_stage);
  if (e->det_ev) (void)hipEventDestroy(e->det_ev);
  if (e->sight_ev) (void)hipEventSynchronize(e->sight_ev);
  if (e->sight_stage) (void)hipHostFree(e->sight_stage);
  if (e->sight_ev) (void)hipEventDestroy(e->sight_ev);
  if (e->x8_plan_stream) {
    (void)hipStreamSynchronize(e->x8_plan_stream);
    (void)hipStreamDestroy(e->x8_plan_stream);
    (void)hipEventDestroy(e->x8_ev_evolved);
    (void)hipEventDestroy(e->x8_ev_planned);
  }
  if (e->ext_stream) {
    (void)hipStreamSynchronize(e->ext_stream);
    (void)hipStreamDestroy(e->ext_stream);
    (void)hipEventDestroy(e->ev_fused_done);
    (void)hipEventDestroy(e->ev_ext_done);
  }
  if (e->fft_plan) hipfftDestroy((hipfftHandle)(uintptr_t)e->fft_plan);
  if (e->sh_plan) hipfftDestroy((hipfftHandle)(uintptr_t)e->sh_plan);
  if (e->shg_plan) hipfftDestroy((hipfftHandle)(uintptr_t)e->shg_plan);
  for (auto& ev : e->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  delete e;
}

int aog_get_info(const aog_env* e, aog_info* out) {
  if (!e || !out) return fail(AOG_ERR_INVALID, "aog_get_info: null argument");
  memset(out, 0, sizeof *out);
  out->abi_version = AOG_ABI_VERSION;
  out->num_envs = e->B;
  out->num_envs_padded = e->Bp;
  out->n_ap = e->n_ap;
  out->n_ap_padded = e->n_ap_pad;
  out->n_modes_padded = e->A_pad;
  out->pixel_chunks = e->geom.n_chunks;
  out->kernel = e->kernel;
  out->n_sums = 2 * (e->MRW + e->MRS);
  out->reserved = (e->ring_direct ? 1 : 0) | (e->obs_sep ? 2 : 0);
  out->device_bytes = e->dev_bytes;
  return AOG_OK;
}

int aog_upload_tables(aog_env* e, const aog_tables* t) {
  if (!e || !t) return fail(AOG_ERR_INVALID, "aog_upload_tables: null argument");
  if (!t->ap_index || !t->modes || !t->gram || !t->wfs_tables || !t->sci_tables || !t->wfs_coef || !t->sci_coef)
    return fail(AOG_ERR_INVALID, "aog_upload_tables: null table pointer");
  HIP_TRY(hipSetDevice(e->device));
  e->reset_obs_valid = false;   // new tables: the cached reset observation was made with the old ones
  e->wf_ready = false;          // and the wavefront fit belongs to the old mode matrix (aog_upload_wavefront_fit)
  e->tomo_ready = false;        // the projection's shapes to the old aperture (aog_upload_wavefront_shapes)
  e->sci_ready = false;         // the science camera's aperture table to the old aperture (aog_upload_science)
  e->grad_ready = false;        // the gradient's operand tables to the old tables (aog_upload_gradient)
  e->pyr_ready = e->pyr_rec_ready = false;   // the pyramid sensor's matrices and mask to the old aperture (aog_upload_pyramid)
  e->gobs_ready = false;        // (and the observation gradient of the separable route with them: aog_upload_gradient_obs)
  const int n_ap = e->n_ap, A = e->A, N2 = e->cfg.n_pupil * e->cfg.n_pupil;
  for (int p = 0; p < n_ap; ++p) {
    if (t->ap_index[p] < 0 || t->ap_index[p] >= N2) return fail(AOG_ERR_INVALID, "aog_upload_tables: ap_index[%d] out of range", p);
    if (p && t->ap_index[p] <= t->ap_index[p - 1]) return fail(AOG_ERR_INVALID, "aog_upload_tables: ap_index must be strictly increasing");
  }
  HIP_TRY(hipMemcpy(e->ap_index, t->ap_index, sizeof(int32_t) * n_ap, hipMemcpyHostToDevice));
  e->ap_index_host.assign(t->ap_index, t->ap_index + n_ap);
  {
    const int Nw = (e->cfg.n_pupil + 31) / 32;
    std::vector<uint32_t> bits((size_t)e->cfg.n_pupil * Nw, 0u);
    for (int p = 0; p < n_ap; ++p) {
      const int f = t->ap_index[p], iy = f / e->cfg.n_pupil, ix = f % e->cfg.n_pupil;
      bits[(size_t)iy * Nw + (ix >> 5)] |= 1u << (ix & 31);
    }
    if (int rc = upload(e, &e->ap_bits, bits, true)) return rc;
  }
  HIP_TRY(hipMemcpy(e->gram, t->gram, sizeof(double) * A * A, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->wfs_coef, t->wfs_coef, sizeof(double) * e->n_out * e->MRW_used * 2, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->sci_coef, t->sci_coef, sizeof(double) * e->MRS_used * 2, hipMemcpyHostToDevice));
  if (e->cfg.precision == AOG_PRECISION_FP64) {
    HIP_TRY(hipMemcpy(e->modes64, t->modes, sizeof(double) * n_ap * A, hipMemcpyHostToDevice));
    const int MR = e->MRW_used + e->MRS_used;
    std::vector<double> tb((size_t)n_ap * MR);
    for (int p = 0; p < n_ap; ++p) {
      for (int m = 0; m < e->MRW_used; ++m) tb[(size_t)p * MR + m] = t->wfs_tables[(size_t)m * n_ap + p];
      for (int m = 0; m < e->MRS_used; ++m) tb[(size_t)p * MR + e->MRW_used + m] = t->sci_tables[(size_t)m * n_ap + p];
    }
    HIP_TRY(hipMemcpy(e->tabs64, tb.data(), sizeof(double) * tb.size(), hipMemcpyHostToDevice));
  } else {
    const int Ap = e->A_pad, MR = e->MRW + e->MRS, TROW = round_up(MR, 4);
    std::vector<float> mf((size_t)e->n_ap_pad * Ap, 0.f);
    std::vector<_Float16> m16((size_t)e->n_ap_pad * Ap * 2, (_Float16)0.f);
    const int nstep = Ap / 16;
    for (int p = 0; p < n_ap; ++p)
      for (int k = 0; k < A; ++k) {
        const float v = (float)t->modes[(size_t)p * A + k];
        mf[(size_t)p * Ap + k] = v;
        // modes16[pt][s][hi|lo][lane = 32*h + i][el], mode k = 16 s + 8 h + el
        _Float16 hi, lo;
        aog::split_f16(v * aog::kModeScale, hi, lo);
        const int pt = p >> 5, i = p & 31, sidx = k >> 4, h = (k >> 3) & 1, el = k & 7;
        const size_t base = (((size_t)pt * nstep + sidx) * 2) * 64 + (h * 32 + i);
        m16[base * 8 + el] = hi;
        m16[(base + 64) * 8 + el] = lo;
      }
    std::vector<float> tf((size_t)e->n_ap_pad * TROW, 0.f);
    auto tab = [&](int m, int p) -> float {
      if (m < e->MRW_used) return (float)t->wfs_tables[(size_t)m * n_ap + p];
      if (m >= e->MRW && m - e->MRW < e->MRS_used) return (float)t->sci_tables[(size_t)(m - e->MRW) * n_ap + p];
      return 0.f;
    };
    for (int p = 0; p < n_ap; ++p)
      for (int m = 0; m < MR; ++m) {
        tf[(size_t)p * TROW + m] = tab(m, p);
      }
    HIP_TRY(hipMemcpy(e->modes_f32, mf.data(), sizeof(float) * mf.size(), hipMemcpyHostToDevice));
    {
      // table-MFMA form: A operand of step s, lane (kg, m), element el <-> pixel i = (el & 3) + 16 s + 8 (el >> 2) + 4 kg of the tile
      std::vector<_Float16> t16((size_t)e->n_ptiles * 2 * 2 * 64 * 8, (_Float16)0.f);
      std::vector<float> st((size_t)e->n_ptiles * 32, 0.f);
      for (int pt = 0; pt < e->n_ptiles; ++pt)
        for (int sidx = 0; sidx < 2; ++sidx)
          for (int kg = 0; kg < 2; ++kg)
            for (int el = 0; el < 8; ++el) {
              const int i = (el & 3) + 16 * sidx + 8 * (el >> 2) + 4 * kg;
              const int p = pt * 32 + i;
              if (p >= n_ap) continue;
              for (int m = 0; m < e->MRW_used && m < 32; ++m) {
                const float v = (float)t->wfs_tables[(size_t)m * n_ap + p];
                const _Float16 hi = (_Float16)v;
                const _Float16 lo = (_Float16)(v - (float)hi);
                const size_t base = ((((size_t)pt * 2 + sidx) * 2) * 64 + (kg * 32 + m)) * 8 + el;
                t16[base] = hi;
                t16[base + (size_t)64 * 8] = lo;
              }
              // science table: register a = 8 s + el of half-wave h = kg
              if (e->MRS_used > 0) st[((size_t)pt * 2 + kg) * 16 + 8 * sidx + el] = (float)t->sci_tables[p];
            }
      HIP_TRY(hipMemcpy(e->tab16, t16.data(), sizeof(_Float16) * t16.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->sci_tile, st.data(), sizeof(float) * st.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(e->modes16, m16.data(), sizeof(_Float16) * m16.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->tabs_f32, tf.data(), sizeof(float) * tf.size(), hipMemcpyHostToDevice));
  }
  if (e->cfg.atm_dynamic && e->cfg.precision == AOG_PRECISION_FAST && e->kernel == AOG_KERNEL_MFMA && !e->psi_ring && !getenv("AOG_DYNAMIC_REPACK")) {
    // ring-direct form: where every packed 4-pixel group of every tile starts on the pupil grid, and where it continues when the
    // aperture's row ends inside it.  A group that would touch three rows (pupils of a dozen pixels) keeps the repack form.
    const int N = e->cfg.n_pupil;
    std::vector<uint32_t> desc((size_t)e->n_ptiles * 8, 4u), cont((size_t)e->n_ptiles * 8, 0u);
    bool ok = N >= 8 && N < 16384;
    for (int pt = 0; pt < e->n_ptiles && ok; ++pt)
      for (int g = 0; g < 4; ++g) {
        bool straddle = false;
        for (int hh = 0; hh < 2; ++hh) {
          const int p0 = 32 * pt + 8 * g + 4 * hh;
          const size_t slot = ((size_t)pt * 2 + hh) * 4 + g;
          if (p0 >= n_ap) continue;   // padding group: reads logical (0, 0), its table rows are zero
          const int f0 = t->ap_index[p0], iy = f0 / N, ix = f0 % N;
          int k = 1;
          while (k < 4 && p0 + k < n_ap && t->ap_index[p0 + k] == f0 + k && ix + k < N) ++k;
          if (k < 4 && p0 + k >= n_ap) k = 4;   // the batch of pixels ends here: the rest of the group is padding
          desc[slot] = ((uint32_t)iy << 18) | ((uint32_t)ix << 4) | (uint32_t)k;
          if (k < 4) {
            const int f2 = t->ap_index[p0 + k], iy2 = f2 / N, ix2 = f2 % N;
            for (int q = k + 1; q < 4 && p0 + q < n_ap; ++q) ok = ok && t->ap_index[p0 + q] == f2 + (q - k) && ix2 + (q - k) < N;
            cont[slot] = ((uint32_t)iy2 << 18) | ((uint32_t)((ix2 - k + N) % N) << 4);
            straddle = true;
          }
        }
        if (straddle)
          for (int hh = 0; hh < 2; ++hh) desc[((size_t)pt * 2 + hh) * 4 + g] |= 8u;
      }
    if (ok) {
      int rc;
      if ((rc = upload(e, &e->quad_desc, desc)) != AOG_OK) return rc;
      if ((rc = upload(e, &e->quad_cont, cont)) != AOG_OK) return rc;
      if ((rc = dev_alloc(e, &e->psi_ring, (size_t)e->B * N * (N + 4), true)) != AOG_OK) return rc;
      e->ring_direct = true;
    }
  }
  if (t->focal_m1 && t->focal_m2 && t->n_focal > 0 && !e->focal_m1) {
    const int N = e->cfg.n_pupil, nf = t->n_focal;
    int rc;
    if ((rc = upload(e, &e->focal_m1, t->focal_m1, (size_t)nf * N * 2)) != AOG_OK) return rc;
    if ((rc = upload(e, &e->focal_m2, t->focal_m2, (size_t)nf * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->focal_E, (size_t)N * N * 2)) != AOG_OK) return rc;
    if ((rc = dev_alloc(e, &e->focal_T, (size_t)nf * N * 2)) != AOG_OK) return rc;
    if (e->cfg.precision == AOG_PRECISION_FAST) {   // split-f16 operand tables of the batched matrix-core path (k_focal_pass1 / k_focal_pass2)
      std::vector<_Float16> m1s, m2s;
      e->focal_unscale = mft_operand_tables(t->focal_m1, t->focal_m2, N, nf, mft_geom_wide(N, round_up(nf, 128)), m1s, m2s);
      if ((rc = upload(e, &e->focal_m1s, m1s)) != AOG_OK) return rc;
      if ((rc = upload(e, &e->focal_m2s, m2s)) != AOG_OK) return rc;
      if ((rc = upload(e, &e->focal_ap_yx, ap_yx_table(e), true)) != AOG_OK) return rc;
    }
    e->n_focal = nf;
  }
  e->tables_ready = true;
  return AOG_OK;
}

int aog_set_screens_f64(aog_env* e, const double* psi, int first, int count, void* stream) {
  if (int rc = set_screens<double>(e, psi, first, count, static_cast<hipStream_t>(stream))) return rc;
  return clear_poison_if_whole(e, first, count, static_cast<hipStream_t>(stream));
}

int aog_set_screens_f32(aog_env* e, const float* psi, int first, int count, void* stream) {
  if (int rc = set_screens<float>(e, psi, first, count, static_cast<hipStream_t>(stream))) return rc;
  return clear_poison_if_whole(e, first, count, static_cast<hipStream_t>(stream));
}

int aog_set_rng_seed(aog_env* e, uint64_t seed) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_set_rng_seed: null handle");
  if (int rcp = refuse_pre_evolved(e, "aog_set_rng_seed")) return rcp;   // (the extrusion launched ahead already drew from the old seed)
  if (int rcd = x8_drop_ahead(e)) return rcd;   // (work done ahead for the next step read the state this call changes)
  e->rng_seed = seed;
  return AOG_OK;
}

int aog_set_detector(aog_env* e, const double* photons_host, const double* read_noise_host, const double* background_host, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_set_detector: null handle");
  if (!photons_host) {   // back to the noise-free kernels: today's code, today's bits
    e->det_on = false;
    return AOG_OK;
  }
  if (!read_noise_host || !background_host) return fail(AOG_ERR_INVALID, "aog_set_detector: read_noise / background are NULL beside photons");
  for (int b = 0; b < e->B; ++b) {
    if (!(photons_host[b] > 0) || !std::isfinite(photons_host[b]))
      return fail(AOG_ERR_INVALID, "aog_set_detector: photons[%d] = %g is not finite and > 0", b, photons_host[b]);
    if (!(read_noise_host[b] >= 0) || !std::isfinite(read_noise_host[b]))
      return fail(AOG_ERR_INVALID, "aog_set_detector: read_noise[%d] = %g is not finite and >= 0", b, read_noise_host[b]);
    if (!(background_host[b] >= 0) || !std::isfinite(background_host[b]))
      return fail(AOG_ERR_INVALID, "aog_set_detector: background[%d] = %g is not finite and >= 0", b, background_host[b]);
  }
  // the table route's epilogue keeps the noisy observation in a second LDS plane beside the clean powers
  const size_t lds = epilogue_lds(e, true);
  if (lds > kLdsBytes)
    return fail(AOG_ERR_UNSUPPORTED, "aog_set_detector: the epilogue would need %zu bytes of LDS (%zu without a detector + %zu for the noisy plane of %d "
                "observations x %d envs) > %zu", lds, epilogue_lds(e, false), lds - epilogue_lds(e, false), e->n_obs_tab, aog::kEpiEnvs, kLdsBytes);
  HIP_TRY(hipSetDevice(e->device));
  // (each piece on its own: a call that failed half way leaves nothing the next one would take for complete)
  if (!e->det_par)
    if (int rc = dev_alloc(e, &e->det_par, (size_t)3 * e->B)) return rc;
  if (!e->det_stage) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->det_stage), sizeof(double) * 3 * e->B, hipHostMallocDefault));
  if (!e->det_ev) HIP_TRY(hipEventCreateWithFlags(&e->det_ev, hipEventDisableTiming));
  HIP_TRY(hipEventSynchronize(e->det_ev));   // (the previous copy out of the staging buffer; long done in practice)
  const size_t B = (size_t)e->B;
  std::copy(photons_host, photons_host + B, e->det_stage);
  std::copy(read_noise_host, read_noise_host + B, e->det_stage + B);
  std::copy(background_host, background_host + B, e->det_stage + 2 * B);
  HIP_TRY(hipMemcpyAsync(e->det_par, e->det_stage, sizeof(double) * 3 * B, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
  HIP_TRY(hipEventRecord(e->det_ev, static_cast<hipStream_t>(stream)));
  e->det_on = true;
  return AOG_OK;
}

int aog_get_screens_f64(aog_env* e, double* psi_dev, int first, int count, void* stream) {
  if (!e || !psi_dev) return fail(AOG_ERR_INVALID, "aog_get_screens_f64: null argument");
  if (!e->screens_ready) return fail(AOG_ERR_STATE, "aog_get_screens_f64 before any screen was installed");
  if (int rc = refuse_pre_evolved(e, "aog_get_screens_f64")) return rc;
  if (int rc = check_env_range("aog_get_screens_f64", first, count, e->B)) return rc;
  if (count == 0) return AOG_OK;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = e->cfg.n_pupil;
  const size_t n = (size_t)count * N * N;
  if (e->cfg.atm_dynamic) {
    if (int rcu = unroll_master(e, psi_dev, first, count, s)) return rcu;
  } else {
    HIP_TRY(hipMemsetAsync(psi_dev, 0, sizeof(double) * n, s));
    const bool fast = e->cfg.precision == AOG_PRECISION_FAST;
    hipLaunchKernelGGL(aog::k_screens_from_store, dim3((e->n_ap + 255) / 256, count), dim3(256), 0, s, fast ? e->psi_tile : nullptr,
                       fast ? nullptr : e->psi64, e->ap_index, psi_dev, first, e->n_ap, e->n_ptiles, N * N, 2.0 * M_PI * e->cfg.wavelength_wfs);
  }
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

extern "C++" {
namespace {
struct StatePart {
  void* ptr;
  size_t bytes;
};
std::vector<StatePart> state_parts(const aog_env* e) {
  std::vector<StatePart> v;
  const size_t N2 = (size_t)e->cfg.n_pupil * e->cfg.n_pupil;
  auto add = [&](void* p, size_t b) { if (p && b) v.push_back({p, b}); };
  add(e->act_dm, sizeof(double) * e->B * e->A);
  add(e->t_render, sizeof(int32_t) * e->B);
  add(e->screen_gen, sizeof(uint32_t) * e->B);
  if (e->ring_direct) {
    // (the fp32 layouts of a ring-direct handle are functions of the master screens, origins and reference pistons saved below)
  } else if (e->cfg.precision == AOG_PRECISION_FAST) {
    add(e->psi_tile, sizeof(float) * (size_t)e->n_etiles * e->n_ptiles * 1024);
    add(e->psi_rev, sizeof(float) * (size_t)e->n_quads * e->Bp * 4);
  } else {
    add(e->psi64, sizeof(double) * (size_t)e->B * e->n_ap);
  }
  if (e->cfg.atm_dynamic) {
    add(e->psi_master, sizeof(double) * e->B * N2);
    add(e->origin, sizeof(int32_t) * 2 * e->B);
    add(e->ext_counter, sizeof(uint32_t) * e->B);
    add(e->psi_offset, sizeof(double) * e->B);
    add(e->psi_sum, sizeof(double) * e->B);
  }
  if (e->sh_ready) add(e->sh_act, sizeof(double) * e->B * e->A);
  return v;
}
}  // namespace
}  // extern "C++"

namespace {
struct StateTail {  // host-side counters that steer the device RNG streams; stored in the last 256 bytes of the blob
  int64_t timestep;
  uint64_t rng_seed;
  uint32_t sh_calls, steps_since_reset;
  uint64_t obs_frame;   // (blobs written before the detector existed left these bytes unwritten: such a blob restores an arbitrary frame count,
                        // which only matters once a detector is switched on — the stream then starts wherever the count stands)
  uint64_t pyr_frame;   // the pyramid sensor's photon stream (blobs written before it was saved read 0: what they ran with after an upload)
};
static_assert(sizeof(StateTail) <= 256, "the state blob reserves 256 bytes for the tail");
}  // namespace

int64_t aog_state_bytes(const aog_env* e) {
  if (!e) return -1;
  int64_t n = 256;
  for (const auto& p : state_parts(e)) n += (int64_t)((p.bytes + 255) / 256 * 256);
  return n;
}

int aog_get_state(aog_env* e, void* blob_dev, int64_t* timestep_out, void* stream) {
  if (!e || !blob_dev) return fail(AOG_ERR_INVALID, "aog_get_state: null argument");
  if (int rc = refuse_pre_evolved(e, "aog_get_state")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  size_t off = 0;
  for (const auto& p : state_parts(e)) {
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(blob_dev) + off, p.ptr, p.bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    off += (p.bytes + 255) / 256 * 256;
  }
  union {   // the whole reserved tail is written: fields added later read zero from blobs of today
    StateTail tail;
    char bytes[256];
  } t{};
  memset(t.bytes, 0, sizeof t.bytes);
  t.tail = StateTail{e->timestep, e->rng_seed, e->sh_calls, (uint32_t)e->steps_since_reset, e->obs_frame, e->pyr_frame};
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  HIP_TRY(hipMemcpy(static_cast<char*>(blob_dev) + off, t.bytes, sizeof t.bytes, hipMemcpyHostToDevice));
  if (timestep_out) *timestep_out = e->timestep;
  return AOG_OK;
}

int aog_set_state(aog_env* e, const void* blob_dev, int64_t timestep, void* stream) {
  if (!e || !blob_dev) return fail(AOG_ERR_INVALID, "aog_set_state: null argument");
  if (!e->tables_ready) return fail(AOG_ERR_STATE, "aog_set_state before aog_upload_tables");
  e->pro_pending = false;   // (a restored state replaces the mirror: a pending pipelined action is forgotten)
  e->reset_obs_valid = false;   // (and the screens: the cached reset observation is of the old ones)
  HIP_TRY(hipSetDevice(e->device));
  if (e->pre_evolved) {   // a restored state replaces everything the pending extrusion touches: let it finish, then forget it
    HIP_TRY(hipStreamSynchronize(e->ext_stream));
    e->pre_evolved = false;
  }
  if (int rcd = x8_drop_ahead(e)) return rcd;   // (likewise what the int8 extrusion prepared ahead)
  hipStream_t s = static_cast<hipStream_t>(stream);
  size_t off = 0;
  for (const auto& p : state_parts(e)) {
    HIP_TRY(hipMemcpyAsync(p.ptr, static_cast<const char*>(blob_dev) + off, p.bytes, hipMemcpyDeviceToDevice, s));
    off += (p.bytes + 255) / 256 * 256;
  }
  StateTail tail{};
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(&tail, static_cast<const char*>(blob_dev) + off, sizeof tail, hipMemcpyDeviceToHost));
  e->timestep = timestep;
  e->rng_seed = tail.rng_seed;
  e->sh_calls = tail.sh_calls;
  e->steps_since_reset = tail.steps_since_reset;
  e->obs_frame = tail.obs_frame;
  e->pyr_frame = tail.pyr_frame;   // (aog_upload_pyramid restarts the count: a sensor is uploaded before the state is restored, not after)
  e->sh_sums_ready = false;
  if (poisoned(e))   // a restored state replaces every screen: the handle is usable again
    if (int rc = clear_poison(e)) return rc;
  if (e->ring_direct) {
    int rc = ring_from_master(e, 0, e->B, 1, s);
    if (rc != AOG_OK) return rc;
  }
  if (int rc = load_actuators(e, s, {e->act_rev, e->act16, nullptr})) return rc;   // derived operand layouts follow the restored actuators
  e->screens_ready = true;
  return AOG_OK;
}

int aog_get_phase_screen(aog_env* e, int env_index, float* phase_dev, void* stream) {
  if (!e || !phase_dev) return fail(AOG_ERR_INVALID, "aog_get_phase_screen: null argument");
  if (!e->screens_ready) return fail(AOG_ERR_STATE, "aog_get_phase_screen before aog_set_screens");
  if (e->cfg.precision != AOG_PRECISION_FAST) return fail(AOG_ERR_UNSUPPORTED, "aog_get_phase_screen: fast precision handles only");
  if (int rc = check_env_range("aog_get_phase_screen", env_index, 1, e->B)) return rc;
  if (int rcp = refuse_pre_evolved(e, "aog_get_phase_screen")) return rcp;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t N2 = (size_t)e->cfg.n_pupil * e->cfg.n_pupil;
  if (int rct = ensure_tiles(e, s)) return rct;
  HIP_TRY(hipMemsetAsync(phase_dev, 0, sizeof(float) * N2, s));
  hipLaunchKernelGGL(aog::k_phase_screen, dim3((e->n_ap + 255) / 256), dim3(256), 0, s, e->psi_tile, e->ap_index, phase_dev, env_index, e->n_ap,
                     e->n_ptiles);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_set_return_accumulator(aog_env* e, float* returns_dev) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_set_return_accumulator: null handle");
  e->ret_acc = returns_dev;
  return AOG_OK;
}

int aog_device_status(aog_env* e, int32_t* status_out) {
  if (!e || !status_out) return fail(AOG_ERR_INVALID, "aog_device_status: null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  int v[16];
  HIP_TRY(hipMemcpy(v, e->dev_status, sizeof v, hipMemcpyDeviceToHost));
  *status_out = v[0] | poisoned(e);
#ifdef AOG_DEV
  if (getenv("AOG_X8_DEV") && (atoi(getenv("AOG_X8_DEV")) & 1024)) {
    fprintf(stderr, "[aogym] k_x8_product: cycles per step max %d min %d, most steps %d, workgroups %d; 10 ns ticks from the first workgroup's start: last start %d, last loop end %d, last end %d; mean start-to-loop-end %d\n", v[8], v[9], v[10], v[11], v[3] - v[2], v[4] - v[2], v[5] - v[2], v[11] ? v[6] / v[11] : 0);
    if (const char* path = getenv("AOG_X8_DEV_DUMP")) {   // per-workgroup records: steps | k << 8 | phase << 12 | xcc << 16 | hw cu/sh/se << 20, cycles per step, start, loop end (10 ns ticks)
      static int rec[4 * 2048];
      HIP_TRY(hipMemcpy(rec, e->dev_status + 16, sizeof rec, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(path, "w")) {
        for (int w = 0; w < v[12] && w < 2048; ++w)
          fprintf(f, "%d %d %d %d %d %d %d %d\n", rec[4 * w] & 255, (rec[4 * w] >> 8) & 15, (rec[4 * w] >> 12) & 1, (rec[4 * w] >> 16) & 15, (rec[4 * w] >> 20) & 255, rec[4 * w + 1], rec[4 * w + 2] - v[2], rec[4 * w + 3] - v[2]);
        fclose(f);
      }
    }
    const int z6[6] = {1 << 30, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(e->dev_status + 2, z6, sizeof z6, hipMemcpyHostToDevice));
    const int init[8] = {0, 1 << 30, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(e->dev_status + 8, init, sizeof init, hipMemcpyHostToDevice));
  }
#endif
  if (getenv("AOG_EXTRUDE_TIMING")) {   // developer aid: phase clocks (10 ns ticks) of workgroup 0 of k_extrude16_split
    if (v[1]) fprintf(stderr, "[aogym] extrude16_split WG0 ticks: gather %d noise %d compute %d (matrix passes %d, exchange %d) barrier %d rounds %d matrix passes run %d, shader clocks in them / 16: %d\n", v[4], v[5], v[6], v[9], v[10], v[7], v[8], v[11], v[12]);
    const int one = 1;
    HIP_TRY(hipMemcpy(e->dev_status + 1, &one, sizeof one, hipMemcpyHostToDevice));
  }
  return AOG_OK;
}

int aog_get_actuators(aog_env* e, double* act_dev, void* stream) {
  if (!e || !act_dev) return fail(AOG_ERR_INVALID, "aog_get_actuators: null argument");
  if (int rc = refuse_pre_evolved(e, "aog_get_actuators")) return rc;   // (pipelined stepping: the mirror already holds the next action)
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(act_dev, e->act_dm, sizeof(double) * e->B * e->A, hipMemcpyDeviceToDevice,
                         static_cast<hipStream_t>(stream)));
  return AOG_OK;
}

int aog_set_actuators(aog_env* e, const double* act_dev, void* stream) {
  if (!e || !act_dev) return fail(AOG_ERR_INVALID, "aog_set_actuators: null argument");
  e->pro_pending = false;   // (whatever a pipelined step had loaded is replaced)
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(e->act_dm, act_dev, sizeof(double) * e->B * e->A, hipMemcpyDeviceToDevice, s));
  return load_actuators(e, s, {e->act_rev, e->act16, nullptr});
}

}  // extern "C"

namespace {
// the checks of aog_reset_act / aog_step_act that concern the policy, made before the call changes anything; fills the tail's arguments
int step_act_tail(const aog_env* e, const aog_actor* net, const char* who, uint16_t* obs, float* action_out, float* log_prob_out, float* mean_out,
                  const aog_action_noise* noise, ActTail* t) {
  if (!e || !net || !obs || !action_out || !log_prob_out) return fail(AOG_ERR_INVALID, "%s: null argument", who);
  if (int rc = action_noise_args(noise, who, &t->nz, &t->noisy)) return rc;
  if (net->batch != e->B || net->state_dim != e->n_obs || net->act_dim != e->A)
    return fail(AOG_ERR_INVALID, "%s: the actor (batch %d, state_dim %d, act_dim %d) does not fit the handle (batch %d, obs_dim^2 %d, n_modes %d)", who,
                net->batch, net->state_dim, net->act_dim, e->B, e->n_obs, e->A);
  if (int rc = actor_args(net, who, &t->a, &t->lds)) return rc;
  t->a.action = action_out;
  t->a.log_prob = log_prob_out;
  t->a.mean = mean_out;
  // the table route stages the observation from the epilogue's LDS, one element per thread
  if (!e->obs_sep && e->n_obs * aog::kEpiEnvs > aog::kStepActThreads)
    return fail(AOG_ERR_UNSUPPORTED, "%s: %d table-route observations per env exceed the tail's %d staging threads / 16", who, e->n_obs, aog::kStepActThreads);
  const size_t epi = epilogue_lds(e), lds = aog::step_act_lds_bytes(epi, t->lds);
  if (lds > kLdsBytes)
    return fail(AOG_ERR_UNSUPPORTED, "%s: the fused tail needs %zu bytes of LDS (epilogue %zu, of which the detector's noisy plane %zu; policy query %zu, "
                "prologue %zu) > %zu", who, lds, epi, epi - epilogue_lds(e, false), t->lds, (size_t)aog::kStepActProDoubles * sizeof(double), kLdsBytes);
  return AOG_OK;
}

// the whole reset of the envs `mask` selects from the cached observation (k_reset_cached)
int reset_from_cache(aog_env* e, const uint8_t* mask, float* obs_raw, uint16_t* obs, hipStream_t s) {
  const int n = e->B * std::max(e->A_pad, e->n_obs_tab);
  hipLaunchKernelGGL(aog::k_reset_cached, dim3((n + 255) / 256), dim3(256), 0, s, mask, e->act_dm, e->act_rev, e->act16, e->t_render, e->reset_obs_raw,
                     e->reset_obs, obs_raw, obs, e->B, e->A, e->A_pad, e->Bp, e->n_obs_tab);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int reset_impl(aog_env* e, const uint8_t* mask, float* obs_raw, uint16_t* obs, void* stream, const ActTail* tail) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_reset: null handle");
  if (!e->tables_ready || !e->screens_ready) return fail(AOG_ERR_STATE, "aog_reset before aog_upload_tables/aog_set_screens");
  if (e->obs_sep && !e->obs_ready) return fail(AOG_ERR_STATE, "aog_reset on a separable-observation handle before aog_upload_obs_mft");
  if (int rc = check_poisoned(e, "aog_reset")) return rc;
  if (int rc = refuse_pre_evolved(e, "aog_reset")) return rc;
  if (int rcd = x8_drop_ahead(e)) return rcd;   // (work done ahead for the next step read the state this call changes)
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!mask) e->steps_since_reset = 0;
  // The screens of such a handle stay between episodes and its mirror restarts flat: the observation is the same bits every time (float64 sums
  // in a fixed order, no atomics, no noise) until something is installed (reset_obs_valid).  Semi-dynamic handles refill after every
  // regeneration; dynamic, detector, separable-route and policy-tail resets always run the pupil pass.
  const bool cacheable = e->reset_cache && !e->cfg.atm_dynamic && !e->det_on && !e->obs_sep && !tail && e->cfg.flat_mirror_start && e->n_obs_tab > 0;
  if (cacheable && e->reset_obs_valid) {
    if (int rc = reset_from_cache(e, mask, obs_raw, obs, s)) return rc;
    e->obs_frame += 1;
    return AOG_OK;
  }
  const bool fill = cacheable && !mask;   // (a masked reset observes the other envs' mirrors as they stand: nothing to keep)
  if (fill && !e->reset_obs) {
    const size_t n_el = (size_t)e->B * e->n_obs_tab;
    int rca = dev_alloc(e, &e->reset_obs_raw, n_el, false);
    if (rca != AOG_OK || (rca = dev_alloc(e, &e->reset_obs, n_el, false)) != AOG_OK) return rca;
  }
  const int n = e->B * e->A;
  hipLaunchKernelGGL(aog::k_reset_state, dim3((n + 255) / 256), dim3(256), 0, s, mask, e->act_dm, e->t_render, e->B, e->A, e->cfg.flat_mirror_start);
  int rc = load_actuators(e, s, {e->act_rev, e->act16, nullptr});
  if (rc != AOG_OK || (rc = launch_fused(e, s)) != AOG_OK) return rc;
  if ((rc = launch_obs(e, s, obs_raw, obs, mask)) != AOG_OK) return rc;
  if (fill) {   // the epilogue writes the cache, and the launch of every later reset hands it to the caller
    rc = launch_epilogue(e, false, e->reset_obs_raw, e->reset_obs, nullptr, nullptr, nullptr, nullptr, s);
    if (rc == AOG_OK) rc = reset_from_cache(e, nullptr, obs_raw, obs, s);
    e->reset_obs_valid = rc == AOG_OK;
  } else {
    rc = launch_epilogue(e, false, obs_raw, obs, nullptr, nullptr, nullptr, nullptr, s, nullptr, tail, mask);
  }
  if (rc == AOG_OK && tail) e->pro_pending = true;   // (the mirror holds the first action: aog_step_act(action = NULL) steps it)
  if (rc == AOG_OK) e->obs_frame += 1;
  return rc;
}

int step_body(aog_env* e, const float* action, const float* action_next, bool pipelined, float* obs_raw, uint16_t* obs, float* reward,
              uint8_t* done, float* power, float* strehl, void* stream, bool* mutated, const ActTail* tail, int* queried) {
  if (!e || (!action && !(tail && e->pro_pending))) return fail(AOG_ERR_INVALID, "aog_step: null argument");
  if (!pipelined && !tail && e->pro_pending)
    return fail(AOG_ERR_STATE, "aog_step: a pipelined step has already loaded the next action (continue with aog_step_pipelined)");
  if (pipelined && e->lookahead) return fail(AOG_ERR_UNSUPPORTED, "aog_step_pipelined: not together with aog_set_lookahead");
  if (!e->tables_ready || !e->screens_ready) return fail(AOG_ERR_STATE, "aog_step before aog_upload_tables/aog_set_screens");
  if (e->obs_sep && !e->obs_ready) return fail(AOG_ERR_STATE, "aog_step on a separable-observation handle before aog_upload_obs_mft");
  if (int rc = check_poisoned(e, "aog_step")) return rc;
  if (e->cfg.reward_type == AOG_REWARD_SMF_SSIM && e->n_obs < 7)
    return fail(AOG_ERR_INVALID, "win_size exceeds image extent (smf_ssim needs obs_dim**2 >= 7; AO_env.py:495)");
  if (e->cfg.atm_dynamic && e->pre_evolved && e->next_noise)
    return fail(AOG_ERR_STATE, "aog_step: extrusion normals were supplied for a step whose extrusion already ran (lookahead draws from the device "
                "stream; switch it off for host-supplied normals)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  *mutated = true;   // from here on a failure leaves counters, ring and mirror out of step with each other: step_impl poisons the handle
  e->timestep += 1;  // AO_env.py:123
  e->steps_since_reset += 1;
  bool join_ext = false;
  e->sh_sums_ready = false;   // (an aog_sh_image(NULL) not followed by its aog_sh_update is void once the env has stepped)
  if (e->cfg.atm_dynamic) {
    if (e->pre_evolved) {   // the previous step launched this step's extrusion on the library's stream: join it
      join_ext = true;   // (joined just ahead of the fused kernel: the prologue does not read the screens)
      e->pre_evolved = false;
    } else {
      int rce = evolve_layer(e, s, e->timestep);
      if (rce != AOG_OK) return rce;
    }
  }
  if (!e->pro_pending) {   // (pipelined: the previous call's last launch already turned this step's action into actuators)
    hipLaunchKernelGGL(join_ext ? aog::k_prologue<false> : aog::k_prologue<true>, dim3((e->B + aog::kProEnvs - 1) / aog::kProEnvs), dim3(64 * aog::kProEnvs), 0, s,
                       prologue_args(e, action));
    HIP_TRY(hipGetLastError());
  }
  e->pro_pending = false;
  if (join_ext) HIP_TRY(hipStreamWaitEvent(s, e->ev_ext_done, 0));
  int rc = launch_fused(e, s);
  if (rc != AOG_OK) return rc;
  // separable observation route: its passes read this step's screens and actuators (their own operand copies), so they run here — before the
  // extrusion of step t + 1 is released below and before the epilogue, which reads their powers and may carry the next step's prologue
  if ((rc = launch_obs(e, s, obs_raw, obs)) != AOG_OK) return rc;
  // lookahead: step t + 1's wind shift needs nothing from this step's outputs (AO_env.py:125 vs :132-142), only that the fused kernel (and the
  // separable observation passes) have finished reading the screens.  Not on an episode's last step: reset() observes the atmosphere as this
  // step left it (AO_env.py:84).
  if (e->cfg.atm_dynamic && e->lookahead && !e->next_noise && e->steps_since_reset < e->cfg.max_steps) {
    HIP_TRY(hipEventRecord(e->ev_fused_done, s));
    HIP_TRY(hipStreamWaitEvent(e->ext_stream, e->ev_fused_done, 0));
    if (int rce = evolve_layer(e, e->ext_stream, e->timestep + 1)) return rce;
    HIP_TRY(hipEventRecord(e->ev_ext_done, e->ext_stream));
    e->pre_evolved = true;
  }
  // aog_step_act: the policy rides with the epilogue unless this is the episode's last step (the next one begins with a reset)
  const bool query = tail && e->steps_since_reset < e->cfg.max_steps;
  const int rce = launch_epilogue(e, true, obs_raw, obs, reward, done, power, strehl, s, pipelined ? action_next : nullptr, query ? tail : nullptr);
  if (rce == AOG_OK && ((pipelined && action_next) || query)) e->pro_pending = true;
  if (rce == AOG_OK && query && queried) *queried = 1;
  if (rce == AOG_OK) e->obs_frame += 1;
  return rce;
}

int step_impl(aog_env* e, const float* action, const float* action_next, bool pipelined, float* obs_raw, uint16_t* obs, float* reward,
              uint8_t* done, float* power, float* strehl, void* stream, const ActTail* tail = nullptr, int* queried = nullptr) {
  bool mutated = false;
  const int rc = step_body(e, action, action_next, pipelined, obs_raw, obs, reward, done, power, strehl, stream, &mutated, tail, queried);
  // A launch or a dynamic-LDS request that fails AFTER the step counters moved (and perhaps after the next extrusion was queued) leaves the
  // handle's counters, screens and mirror inconsistent: mark it unusable (bit 1 of the status word; cleared like a barrier timeout, by
  // installing screens for the whole batch or restoring a saved state) instead of letting later steps run on it.
  if (rc != AOG_OK && mutated && e) poison(e, 2);
  return rc;
}
}  // namespace

extern "C" {

int aog_reset(aog_env* e, const uint8_t* mask, float* obs_raw, uint16_t* obs, void* stream) { return reset_impl(e, mask, obs_raw, obs, stream, nullptr); }

int aog_reset_act_noise(aog_env* e, const aog_actor* net, float* obs_raw, uint16_t* obs, float* action_out, float* log_prob_out, float* mean_out,
                        const aog_action_noise* noise, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_reset_act: null handle");
  if (int rc = refuse_pre_evolved(e, "aog_reset_act")) return rc;
  ActTail t{};
  if (int rc = step_act_tail(e, net, "aog_reset_act", obs, action_out, log_prob_out, mean_out, noise, &t)) return rc;
  return reset_impl(e, nullptr, obs_raw, obs, stream, &t);
}
int aog_reset_act(aog_env* e, const aog_actor* net, float* obs_raw, uint16_t* obs, float* action_out, float* log_prob_out, float* mean_out,
                  void* stream) {
  return aog_reset_act_noise(e, net, obs_raw, obs, action_out, log_prob_out, mean_out, nullptr, stream);
}

int aog_step(aog_env* e, const float* action, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done, float* power,
             float* strehl, void* stream) {
  return step_impl(e, action, nullptr, false, obs_raw, obs, reward, done, power, strehl, stream);
}
int aog_step_pipelined(aog_env* e, const float* action, const float* action_next, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done,
                       float* power, float* strehl, void* stream) {
  return step_impl(e, action, action_next, true, obs_raw, obs, reward, done, power, strehl, stream);
}
int aog_step_act_noise(aog_env* e, const aog_actor* net, const float* action, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done,
                       float* power, float* strehl, float* action_out, float* log_prob_out, float* mean_out, int* queried,
                       const aog_action_noise* noise, void* stream) {
  if (queried) *queried = 0;
  if (!e) return fail(AOG_ERR_INVALID, "aog_step_act: null handle");
  if (!action && !e->pro_pending)
    return fail(AOG_ERR_INVALID, "aog_step_act: action = NULL but no action is pending (the first step after a plain aog_reset needs its action)");
  if (action && e->pro_pending)
    return fail(AOG_ERR_INVALID, "aog_step_act: an action is pending (from aog_reset_act / aog_step_act / aog_step_pipelined): pass action = NULL");
  ActTail t{};
  if (int rc = step_act_tail(e, net, "aog_step_act", obs, action_out, log_prob_out, mean_out, noise, &t)) return rc;
  return step_impl(e, action, nullptr, false, obs_raw, obs, reward, done, power, strehl, stream, &t, queried);
}
int aog_step_act(aog_env* e, const aog_actor* net, const float* action, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done, float* power,
                 float* strehl, float* action_out, float* log_prob_out, float* mean_out, int* queried, void* stream) {
  return aog_step_act_noise(e, net, action, obs_raw, obs, reward, done, power, strehl, action_out, log_prob_out, mean_out, queried, nullptr, stream);
}
// the checks of aog_reset_spgd / aog_step_spgd that concern the controller, made before the call changes anything
static int step_spgd_tail(const aog_env* e, const aog_spgd* g, const char* who, const float* action_out) {
  if (!e || !g || !action_out) return fail(AOG_ERR_INVALID, "%s: null argument", who);
  if (!e->cfg.sh_operation)
    return fail(AOG_ERR_INVALID, "%s: the handle was created without sh_operation: its action is rescaled to a fixed surface rms, so a perturbation "
                "amplitude means nothing there", who);
  if (g->cfg.act_dim != e->A) return fail(AOG_ERR_INVALID, "%s: the controller's act_dim %d is not the handle's n_modes %d", who, g->cfg.act_dim, e->A);
  if (g->cfg.num_envs != e->B) return fail(AOG_ERR_INVALID, "%s: the controller's num_envs %d is not the handle's %d", who, g->cfg.num_envs, e->B);
  if (g->cfg.env_id_base != e->cfg.env_id_base || g->state.device != e->device)
    return fail(AOG_ERR_INVALID, "%s: the controller (env_id_base %d, device %d) does not belong to the handle (env_id_base %d, device %d)", who,
                g->cfg.env_id_base, g->state.device, e->cfg.env_id_base, e->device);
  const size_t lds = aog::step_spgd_lds_bytes(epilogue_lds(e));
  if (lds > kLdsBytes) return fail(AOG_ERR_UNSUPPORTED, "%s: the fused tail needs %zu bytes of LDS > %zu", who, lds, kLdsBytes);
  return AOG_OK;
}
int aog_reset_spgd(aog_env* e, aog_spgd* g, float* obs_raw, uint16_t* obs, float* action_out, void* stream) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_reset_spgd: null handle");
  if (int rc = refuse_pre_evolved(e, "aog_reset_spgd")) return rc;
  if (int rc = step_spgd_tail(e, g, "aog_reset_spgd", action_out)) return rc;
  ActTail t{};
  t.spgd = true;
  // (the reset's k_reset_state has flattened the mirror, or left it: the query starts u from what the prologue would replace)
  t.sp = spgd_args(g, true, nullptr, nullptr, e->cfg.flat_mirror_start ? nullptr : e->act_dm, action_out);
  return reset_impl(e, nullptr, obs_raw, obs, stream, &t);
}
int aog_step_spgd(aog_env* e, aog_spgd* g, const float* action, float* obs_raw, uint16_t* obs, float* reward, uint8_t* done, float* power,
                  float* strehl, float* action_out, int* queried, void* stream) {
  if (queried) *queried = 0;
  if (!e) return fail(AOG_ERR_INVALID, "aog_step_spgd: null handle");
  if (!action && !e->pro_pending)
    return fail(AOG_ERR_INVALID, "aog_step_spgd: action = NULL but no action is pending (the first step after a plain aog_reset needs its action)");
  if (action && e->pro_pending)
    return fail(AOG_ERR_INVALID, "aog_step_spgd: an action is pending (from aog_reset_spgd / aog_step_spgd / aog_step_pipelined): pass action = NULL");
  if (int rc = step_spgd_tail(e, g, "aog_step_spgd", action_out)) return rc;
  // the query reads the float32 the epilogue stores: an output the caller leaves out goes to the controller's own buffer
  float** sel = g->cfg.metric == AOG_SPGD_POWER ? &power : g->cfg.metric == AOG_SPGD_STREHL ? &strehl : &reward;
  if (!*sel) *sel = g->metric;
  ActTail t{};
  t.spgd = true;
  t.sp = spgd_args(g, false, *sel, nullptr, nullptr, action_out);
  return step_impl(e, action, nullptr, false, obs_raw, obs, reward, done, power, strehl, stream, &t, queried);
}
int aog_selftest_sincos(const float* u_dev, float* sin_dev, float* cos_dev, int n, int flavour, void* stream) {
  if (!u_dev || !sin_dev || !cos_dev || n < 0 || flavour < 0 || flavour > 2) return fail(AOG_ERR_INVALID, "aog_selftest_sincos: bad argument");
  if (n == 0) return AOG_OK;
  hipLaunchKernelGGL(aog::k_selftest_sincos, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), u_dev, sin_dev,
                     cos_dev, n, flavour);
  HIP_TRY(hipGetLastError());
  return AOG_OK;
}

int aog_profile_block(aog_env* e, int launches) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_profile_block: null handle");
  if (launches < 1 || launches > 64) return fail(AOG_ERR_INVALID, "aog_profile_block: %d launches per block (1 .. 64)", launches);
  e->profile_block = launches;
  return AOG_OK;
}

int aog_profile_enable(aog_env* e, int enable) {
  if (!e) return fail(AOG_ERR_INVALID, "aog_profile_enable: null handle");
  e->profile = enable != 0;
  e->profile_every = enable > 1 ? enable : 1;
  e->profile_phase = 0;
  e->events_used = 0;
  if (e->profile && e->events.size() < 1024) {
    // event pairs are created here, not inside the caller's timed region (a few microseconds each; the pool still grows on demand)
    HIP_TRY(hipSetDevice(e->device));
    while (e->events.size() < 1024) {
      hipEvent_t a = nullptr, b = nullptr;
      HIP_TRY(hipEventCreate(&a));
      HIP_TRY(hipEventCreate(&b));
      e->events.emplace_back(a, b);
    }
    // first use of timed events sets up runtime state (milliseconds): do it here
    float ms = 0;
    HIP_TRY(hipEventRecord(e->events[0].first, nullptr));
    HIP_TRY(hipEventRecord(e->events[0].second, nullptr));
    HIP_TRY(hipEventSynchronize(e->events[0].second));
    HIP_TRY(hipEventElapsedTime(&ms, e->events[0].first, e->events[0].second));
  }
  return AOG_OK;
}

int aog_profile_read(aog_env* e, double* mean_ms, int* launches) {
  if (!e || !mean_ms || !launches) return fail(AOG_ERR_INVALID, "aog_profile_read: null argument");
  HIP_TRY(hipSetDevice(e->device));
  for (int k = 0; k < AOG_PROF_COUNT; ++k) {
    e->prof_ms[k] = 0;
    e->prof_n[k] = 0;
  }
  for (size_t i = 0; i < e->events_used; ++i) {
    HIP_TRY(hipEventSynchronize(e->events[i].second));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->events[i].first, e->events[i].second));
    const int k = i < e->event_kernel.size() ? e->event_kernel[i] : AOG_PROF_FUSED;
    e->prof_ms[k] += ms;
    e->prof_n[k] += 1;
  }
  *launches = e->prof_n[AOG_PROF_FUSED];
  *mean_ms = e->prof_n[AOG_PROF_FUSED] ? e->prof_ms[AOG_PROF_FUSED] / (double)e->prof_n[AOG_PROF_FUSED] : 0.0;
  e->events_used = 0;
  e->profile_phase = 0;   // the next launch opens a timed block: a short measurement after a read still gets its samples
  return AOG_OK;
}

int aog_profile_read_kernel(aog_env* e, int which, double* mean_ms, int* launches) {
  if (!e || !mean_ms || !launches) return fail(AOG_ERR_INVALID, "aog_profile_read_kernel: null argument");
  if (which < 0 || which >= AOG_PROF_COUNT) return fail(AOG_ERR_INVALID, "aog_profile_read_kernel: unknown kernel id %d", which);
  *launches = e->prof_n[which];
  *mean_ms = e->prof_n[which] ? e->prof_ms[which] / (double)e->prof_n[which] : 0.0;
  return AOG_OK;
}

}  // extern "C"
