// The life of a handle that is no aog_env (aog_predictor, aog_telemetry, aog_spgd, aog_link, aog_disturbance, aog_servo), written once:
// null checks by name, create, destroy and the checkpoint calls.  A unit adds its config check, its first fill and its own entry points.
#pragma once
#include "host_common.h"

#include <initializer_list>
#include <utility>

namespace aog_host {

// the first null pointer among an entry point's arguments, by its name in the header (nullptr: none is null)
inline const char* first_null(std::initializer_list<std::pair<const char*, const void*>> args) {
  for (const auto& a : args)
    if (!a.second) return a.first;
  return nullptr;
}
#define REFUSE_NULL(who, ...)                                                                      \
  do {                                                                                             \
    if (const char* name__ = ::aog_host::first_null({__VA_ARGS__}))                                \
      return ::aog_host::fail(AOG_ERR_INVALID, "%s: null argument %s", who, name__);               \
  } while (0)

// What such a handle holds: its config, its records and the further device buffers it owns.  `device` is current whenever a member runs.
template <typename Config>
struct StandaloneHandle {
  Config cfg{};
  RecordStore state;
  std::vector<void*> owned;   // what handle_release frees: a unit allocates every further buffer through own(), never with hipMalloc itself
  hipError_t alloc_state(size_t bytes, bool zero) {
    const hipError_t err = state.alloc(state.device, bytes);
    return err == hipSuccess && zero ? hipMemset(state.ptr, 0, bytes) : err;
  }
  template <typename T>
  hipError_t own(T** p, size_t bytes, bool zero) {
    const hipError_t err = hipMalloc(reinterpret_cast<void**>(p), bytes);
    if (err != hipSuccess) return err;
    owned.push_back(*p);
    return zero ? hipMemset(*p, 0, bytes) : hipSuccess;
  }
};

template <typename H>
void handle_release(H* h) {
  h->state.release();
  for (void* p : h->owned) (void)hipFree(p);
  delete h;
}

// `who`_create: check(cfg) returns AOG_OK or has called fail, before any device work; fill(h) allocates and puts the first values there on
// the null stream, which a caller's non-blocking stream does not wait for — hence the one wait behind it
template <typename H, typename Config, typename Check, typename Fill>
int handle_create(const char* who, const Config* cfg, int device, H** out, Check&& check, Fill&& fill) {
  REFUSE_NULL(who, {"cfg", cfg}, {"out", out});
  *out = nullptr;
  if (int rc = check(cfg)) return rc;
  HIP_TRY(hipSetDevice(device));
  H* h = new H;
  h->cfg = *cfg;
  h->state.device = device;
  hipError_t err = fill(h);
  if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  if (err != hipSuccess) {
    handle_release(h);
    return fail(AOG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
  }
  *out = h;
  return AOG_OK;
}

template <typename H>
void handle_destroy(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->state.device);
  handle_release(h);
}

template <typename H>
int64_t handle_state_bytes(const H* h) {
  return h ? (int64_t)h->state.bytes : 0;
}
// (`name`: the handle's parameter name in the header)
template <typename H>
int handle_get_state(const char* who, const char* name, const H* h, void* blob_dev, void* stream) {
  REFUSE_NULL(who, {name, h}, {"blob_dev", blob_dev});
  return h->state.copy_out(blob_dev, stream);
}
template <typename H>
int handle_set_state(const char* who, const char* name, H* h, const void* blob_dev, void* stream) {
  REFUSE_NULL(who, {name, h}, {"blob_dev", blob_dev});
  return h->state.copy_in(blob_dev, stream);
}

}  // namespace aog_host
