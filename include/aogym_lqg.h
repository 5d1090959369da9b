/* LQG controller (additive in ABI 22; no counterpart in the reference): per env and per mode a Kalman filter on a turbulence-plus-vibration
 * state model that predicts `delay` frames ahead — the classical baseline against narrow vibration lines and loop delay.  A handle of its
 * own, aog_lqg, on the stand-alone handles' lifecycle, independent of any aog_env (as aog_servo, aog_tomo): it turns a [B][A] float64
 * pseudo-open-loop measurement into a [B][A] float64 command.  Declared here and not in aogym.h for the reason aogym_servo.h gives; the
 * streams of its calls are held from tests/test_gpu_lqg.py.  No struct, constant or signature of aogym.h changes.
 *
 * Everything below is per env b and mode j; B = num_envs >= 1, A = act_dim in 1 .. 128, S = n_models in 1 .. 4, n = 2 S, reserved = 0.
 * The struct is five int32 (aog_lqg_config_size); it has no index in aog_struct_size.
 *
 * Model.  The measurement is y_t = sum_s x^(s)_t + w_t, var w = r.  Sub-model s (0: the turbulence, 1 .. S-1: vibration lines) is the
 * AR(2) process x_t = a1_s x_{t-1} + a2_s x_{t-2} + v_t, var v = q_s.  The state is x = (x^(0)_t, x^(0)_{t-1}, x^(1)_t, ...), n entries:
 * A is block-diagonal with the companion blocks [[a1_s, a2_s], [1, 0]], C picks entry 2 s of every block, Q is diagonal with q_s there.
 * The measurement is open loop: the filter does not depend on the command.  What is not modelled: a mirror that answers its command with
 * a first-order response < 1, and a fractional latency (round it up).
 *
 * Records.  Every per-(env, mode) array is laid out [B][row][A], mode innermost: one thread per (env, mode) reads and writes coalesced
 * rows and touches each word once per call.  The rows of an env, 9 S + 4 in all, float64 each:
 *     a [S][2] (a1_s, a2_s) | q [S] | r | K [n] | c_d [n] | convergence | solved (0 or 1) | xhat [n] | command
 * That is also the checkpoint blob, 8 B (9 S + 4) A bytes.  A handle starts as zeros.
 *
 * aog_lqg_set_model copies a_dev [B][S][2][A], q_dev [B][S][A] and r_dev [B][A] (float64 DEVICE arrays) into the selected envs and zeroes
 * their K, c_d, convergence, solved, xhat and command.  It holds no host-side validation of device values: a model that is not finite, is
 * unstable or has r <= 0 surfaces in aog_lqg_solve's convergence figure, as NaN.
 *
 * aog_lqg_solve(delay in 1 .. 4, iterations in 1 .. 4096), one lane per selected (env, mode), P (symmetric, its upper triangle) in
 * registers.  With P(i, k) standing for the stored entry (min, max), sums running left to right from their first term, and every product,
 * sum and quotient one rounded float64 operation, never fused (a host replay, tests/lqg_reference.py, is bit-exact):
 *     P = Q;  t_prev = trace(P) = sum_i P(i, i)
 *     `iterations` times:
 *         pc[i] = sum_s P(i, 2 s)                          s_ = (sum_s pc[2 s]) + r             K[i] = pc[i] / s_
 *         M(i, k) = P(i, k) + (-(K[i] pc[k]))              for i <= k
 *         for blocks s <= t, with m00 = M(2s, 2t), m01 = M(2s, 2t+1), m10 = M(2s+1, 2t) (s = t: M(2s, 2s+1)), m11 = M(2s+1, 2t+1):
 *             n00 = (a1_s m00) + (a2_s m10)                n01 = (a1_s m01) + (a2_s m11)
 *             P'(2s, 2t) = (n00 a1_t) + (n01 a2_t), + q_s when s = t;   P'(2s, 2t+1) = n00;   P'(2s+1, 2t+1) = m00
 *             s < t:  P'(2s+1, 2t) = (m00 a1_t) + (m01 a2_t)
 *         t_prev = t_last;  P = P';  t_last = trace(P)
 *     pc, s_, K once more from the last P: that K is stored
 *     c = C;  `delay` times:  c'[2s] = (c[2s] a1_s) + c[2s+1],  c'[2s+1] = c[2s] a2_s;   c_d = c is stored
 *     convergence = |t_last + (-t_prev)| / t_last;   solved = 1
 *     convergence = NaN unless r > 0 and every sub-model is stable: |a2_s| < 1, a1_s + a2_s < 1, a2_s + (-a1_s) < 1 (the Riccati recursion
 *     itself converges for an unstable model that the measurement observes; a prediction `delay` frames ahead with one is refused here)
 * (the zeros and ones of the companion blocks are used only by leaving out the terms written out above as absent).  convergence_out_dev
 * [B][A] (nullable) receives the figure of the selected envs; rows of the others are not written.  Registers and scratch of the kernel:
 * profiles/lqg.md.
 *
 * aog_lqg_update, one launch, for every selected env whose row y[b][:] is finite and every mode:
 *     e = y + (-(sum_s xhat[2s]));   xp[i] = xhat[i] + (K[i] e);   u = sum_i (c_d[i] xp[i]);   command = u
 *     xhat[2s] = (a1_s xp[2s]) + (a2_s xp[2s+1]);   xhat[2s+1] = xp[2s]
 * under the same rounding rule.  A non-finite y anywhere in a row leaves that whole env untouched.  out_dev [B][A] receives the command of
 * every env as it stands after the call (an env that was left out or frozen: its last command).  AOG_ERR_INVALID unless aog_lqg_solve has
 * run since the last aog_lqg_set_model (after aog_lqg_set_state: unless every env of the blob is solved).
 *
 * aog_lqg_reset zeroes xhat and command of the selected envs; the model and the gains stay.
 *
 * Every call is ordered by the one stream it is given; none waits for the device but aog_lqg_set_state, which copies the blob on `stream`
 * and then WAITS for it: whether the blob is solved comes back to the host.  A resumed handle continues bit-identically without solving
 * again.  An env's results depend on that env's records and inputs alone: handles that hold the parts of a batch reproduce the whole batch
 * bit for bit.  mask_dev: nullable [B] uint8 device array, non-zero = selected.
 *
 * AOG_ERR_INVALID, before any device work, with aog_last_error naming the entry point and the field: a null handle, config or required
 * array; a wrong abi_version, num_envs < 1, act_dim outside 1 .. 128, n_models outside 1 .. 4, reserved != 0; delay outside 1 .. 4,
 * iterations outside 1 .. 4096; aog_lqg_update before aog_lqg_solve. */
#ifndef AOGYM_LQG_H
#define AOGYM_LQG_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_LQG_MAX_ACT = 128, AOG_LQG_MAX_MODELS = 4, AOG_LQG_MAX_DELAY = 4, AOG_LQG_MAX_ITERATIONS = 4096 };

typedef struct aog_lqg aog_lqg;
typedef struct aog_lqg_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, act_dim, n_models;
  int32_t reserved;                     /* 0 */
} aog_lqg_config;
int64_t aog_lqg_config_size(void);
int aog_lqg_create(const aog_lqg_config* cfg, int device, aog_lqg** out);
void aog_lqg_destroy(aog_lqg* lqg);
int aog_lqg_set_model(aog_lqg* lqg, const double* a_dev, const double* q_dev, const double* r_dev, const uint8_t* mask_dev, void* stream);
int aog_lqg_solve(aog_lqg* lqg, int delay, int iterations, double* convergence_out_dev, const uint8_t* mask_dev, void* stream);
int aog_lqg_update(aog_lqg* lqg, const double* y_dev, double* out_dev, const uint8_t* mask_dev, void* stream);
int aog_lqg_reset(aog_lqg* lqg, const uint8_t* mask_dev, void* stream);
int64_t aog_lqg_state_bytes(const aog_lqg* lqg);
int aog_lqg_get_state(aog_lqg* lqg, void* blob_dev, void* stream);
int aog_lqg_set_state(aog_lqg* lqg, const void* blob_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_LQG_H */
