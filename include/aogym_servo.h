/* Mirror servo: loop latency, mirror dynamics, finite stroke and dead actuators between the commanded action and the action the mirror
 * receives (additive in ABI 22; no counterpart in the reference).  A handle of its own, aog_servo, independent of any aog_env (as
 * aog_disturbance, aog_spgd, aog_link): it turns a [B][A] float32 action into a [B][A] float32 action, and whoever owns it steps the env
 * with the result.  Declared here and not in aogym.h so that the rule tests/test_stream_coverage_cpu.py holds aogym.h to is held for this
 * header from files of its own (tests/test_servo_stream_coverage_cpu.py, tests/test_gpu_servo_streams.py).  No struct, constant or
 * signature of aogym.h changes. */
#ifndef AOGYM_SERVO_H
#define AOGYM_SERVO_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_SERVO_MAX_LATENCY = 4, AOG_SERVO_MAX_ACT = 128 };

/* Configuration: B = num_envs >= 1, A = act_dim in 1 .. 128, max_latency in 0 .. 4 (whole frames); R = max_latency + 2 is the depth of
 * the command history.  There is no random stream and therefore no seed and no env id.  The struct is four int32 (16 bytes:
 * aog_servo_config_size); it has no index in aog_struct_size.
 *
 * Parameters (aog_servo_set_params; HOST arrays; a blocking copy that is not ordered behind any stream's pending calls).  Until the
 * first call every env has latency 0, response 1, no stroke limit and no stuck actuator: the identity.
 *   latency[b]         float64, frames, in [0, max_latency]; fractional values allowed
 *   response[b]        float64, in (0, 1]: the share of the way to its command the mirror moves in one frame (1: at once)
 *   stroke[b]          float64, > 0: the drive is clipped to [-stroke, stroke]; +infinity: no limit
 *   stuck[b][j]        uint8, non-zero: actuator j of env b is dead
 *   stuck_value[b][j]  float32, finite: where it sits
 *
 * State.
 *   y[b][j]            float64: the output of the response filter
 *   ring[b][s][j]      float32, s in 0 .. R - 1: the commanded actions, exact copies
 *   n                  one uint64 per HANDLE: the number of aog_servo_apply calls made so far.  Every aog_servo_apply raises it by 1
 *                      whatever its mask; nothing else moves it but aog_servo_set_state.
 * Slot rule: the call that finds the counter at n writes its action to slot n mod R, and a_{n-k}, 0 <= k <= R - 1, stands for
 * ring[b][(n - k) mod R][j] (mathematical mod: slot ((n mod R) + R - k) mod R).  A handle starts with n = 0, y = 0 and a ring of zeros.
 *
 * aog_servo_apply at call n, for every env b the mask selects and every actuator j:
 *   1. ring[b][n mod R][j] = a_n = action_in[b][j]
 *   2. d = floor(latency[b]), f = latency[b] - d (exact).  f == 0: c = a_{n-d}.  Otherwise c = ((1 - f) a_{n-d}) + (f a_{n-d-1}).
 *      (d + 1 <= max_latency = R - 2 whenever f > 0, and d <= R - 2 always: every entry read lies inside the ring.)
 *   3. stroke[b] < +infinity: c = min(max(c, -stroke[b]), stroke[b]) (c < -stroke gives -stroke, then c > stroke gives stroke: a NaN passes)
 *   4. response[b] == 1: y = c.  Otherwise y = y + (response[b] (c - y)).
 *   5. action_out[b][j] = stuck[b][j] ? stuck_value[b][j] : (float)y, rounded to nearest even.
 * The float32 entries of the ring are widened to float64 exactly; 1 - f, the two products, their sum, c - y, its product with response
 * and the sum with y are one rounded float64 operation each, in the order written; nothing is fused.  A host replay is therefore
 * bit-exact, and since env b's result depends on env b's parameters, state and actions and on n alone, handles that hold the parts of a
 * batch and receive the same calls reproduce the whole batch bit for bit.  With latency 0, response 1, no stroke limit and no stuck
 * actuator action_out holds the bits of action_in (a NaN's payload aside).
 *   An env the mask leaves out keeps its ring and its y, and its row of action_out is not written.  The counter moves on all the same:
 * slot n mod R of that env keeps what it held (the env's command of R calls earlier, or 0), and later calls read that as a_n.
 *   aog_servo_reset: ring and y of the selected envs become 0 — the rest command: every entry from before an env's last reset reads as
 * 0.  The counter stays.
 *
 * One thread per (env, actuator), one launch per call; plain vector loads and stores, no atomics, no host synchronisation in
 * aog_servo_reset, aog_servo_apply and aog_servo_get_state; the calls on one handle are ordered by the one stream they are given, in the
 * order the host makes them.  The host keeps the counter and hands it to each launch as an argument (no thread reads a word another
 * thread of its launch writes); the launch's first thread stores n + 1 into the state for aog_servo_get_state.  aog_servo_set_state
 * copies the blob on `stream` and then WAITS for that stream: the host's counter comes back from the blob.
 * mask_dev: nullable [B] uint8 device array, non-zero = selected.  action_in_dev, action_out_dev: [B][A] float32 device arrays; they may
 * be the same array.
 *
 * AOG_ERR_INVALID, before any device work, with aog_last_error naming the entry point and the field: a null handle, config, output or
 * array; a wrong abi_version, num_envs < 1, act_dim outside 1 .. 128, max_latency outside 0 .. 4; a latency outside [0, max_latency], a
 * response outside (0, 1], a stroke that is not > 0 (NaN included), a stuck_value that is not finite. */
typedef struct aog_servo aog_servo;
typedef struct aog_servo_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, act_dim, max_latency;
} aog_servo_config;
int64_t aog_servo_config_size(void);
int aog_servo_create(const aog_servo_config* cfg, int device, aog_servo** out);
void aog_servo_destroy(aog_servo* servo);
int aog_servo_set_params(aog_servo* servo, const double* latency_host, const double* response_host, const double* stroke_host,
                         const uint8_t* stuck_host, const float* stuck_value_host);
int aog_servo_reset(aog_servo* servo, const uint8_t* mask_dev, void* stream);
int aog_servo_apply(aog_servo* servo, const float* action_in_dev, const uint8_t* mask_dev, float* action_out_dev, void* stream);
/* Checkpointing: y [B][A] float64, then the counter (uint64), then ring [B][R][A] float32: 8 B A + 8 + 4 B R A bytes.  A handle of the
 * same configuration and parameters that takes the blob resumes bit-identically. */
int64_t aog_servo_state_bytes(const aog_servo* servo);
int aog_servo_get_state(aog_servo* servo, void* blob_dev, void* stream);
int aog_servo_set_state(aog_servo* servo, const void* blob_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_SERVO_H */
