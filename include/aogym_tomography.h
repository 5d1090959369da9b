/* Tomography (additive in ABI 22; no counterpart in the reference): what a multi-conjugate controller needs on the device.  Two parts.
 * (1) aog_wavefront_project: a front's residual wavefront projected onto shapes of the caller's — an altitude mirror's influence functions
 * seen along a sightline are shifted, cropped footprints that do not lie in the span of the pupil mirror's modes, which is all
 * aog_wavefront_truth projects onto.  (2) aog_tomo_*: a handle of its own that holds the reconstructor matrices and the integrator's
 * command.  Declared here and not in aogym.h for the reason aogym_disturbance.h gives: the stream-coverage rule is held for this header
 * from files of its own (tests/test_tomography_stream_coverage_cpu.py, tests/test_gpu_tomography_streams.py).  No struct, constant or
 * signature of aogym.h changes. */
#ifndef AOGYM_TOMOGRAPHY_H
#define AOGYM_TOMOGRAPHY_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_WAVEFRONT_MAX_SHAPES = 512, AOG_TOMO_MAX_OUT = 576, AOG_TOMO_MAX_INPUTS = 4, AOG_TOMO_MAX_WIDTH = 576 };

/* aog_upload_wavefront_shapes: K shapes over the aperture, shapes_host a HOST array [K][n_ap] float64 (packed aperture pixels, the order
 * of aog_tables.ap_index), 1 <= K <= 512, every value finite.  AOG_ERR_STATE before aog_upload_tables; aog_upload_tables forgets the
 * shapes.  Blocking, like aog_upload_wavefront_fit; a second upload replaces the first (K may change).  Fast handles keep the shapes as
 * split-f16 operands at a scale of this upload's own, the power of two that brings the largest |S| into [2^13, 2^14) (shapes are not of
 * unit size the way the modes are); float64 handles keep them as they are.  The row sums sum_p S[k][p] are formed here in float64.
 *
 * aog_wavefront_project: for every env b and shape k
 *     out[b][k] = sum_p S[k][p] (w_bp - mean_b),    mean_b = (sum_p w_bp) / n_ap,    mean[b] = mean_b  (mean_dev nullable)
 * where w is the residual optical path error in metres over the aperture, exactly the w of aog_wavefront_truth: on fast handles
 * lambda_wfs (psi + M' a) with the phase in revolutions as the step kernels form it, on float64 handles psi64 / 2 pi + 2 (M a).  It is
 * evaluated as  lambda_wfs T_k - rowsum_k mean_b  (T_k = sum_p S[k][p] u_bp) in float64 without a fused multiply-add.  out_dev [B][K]
 * and mean_dev [B] are float64 DEVICE arrays.  Fast handles: T_k on the matrix cores, u and S split into f16 pairs (three products),
 * fp32 sums over a tile of 32 pixels, float64 beyond; the shapes are cut into groups of at most 128 rows, one workgroup per (pixel
 * chunk, env tile, group).  An env's sums depend on nothing but its own column of the operands: a batch split over two handles gives the
 * bits of the whole batch.  Float64 handles: one workgroup per env, within n_ap 2^-53 sum_p |S[k][p]| |w_bp| of any other order.
 * The checks of every off-step instrument apply (AOG_ERR_STATE before tables and screens, without uploaded shapes, on a poisoned handle,
 * while a pipelined step has the next action in the mirror or the atmosphere stands at the next step).  Stream-ordered, no host
 * synchronisation; nothing a step reads is written. */
int aog_upload_wavefront_shapes(aog_env* env, const double* shapes_host, int n_shapes);
int aog_wavefront_project(aog_env* env, double* out_dev, double* mean_dev, void* stream);

/* The reconstructor and integrator: a handle of its own on the stand-alone handles' lifecycle.  B = num_envs >= 1, K = n_out in 1 .. 576,
 * G = n_inputs in 1 .. 4, J_g = width[g] in 1 .. 576 for g < G and 0 beyond, env_id_base >= 0 (kept for symmetry with the other
 * handles: there is no random stream), reserved = 0.  The struct is ten int32 (aog_tomo_config_size); it has no index in aog_struct_size.
 *
 * Buffers: R_g float64 [K][J_g] per input (zeros until aog_tomo_upload), u float64 [B][K] — the command, zero at creation, and the
 * checkpoint blob (8 B K bytes).
 *
 * aog_tomo_upload copies the DEVICE array R_dev [K][J_g] of input g on `stream`.
 *
 * aog_tomo_update, for every env b the mask selects (mask_dev nullable [B] uint8 device array) and every k:
 *     acc = 0;   for g = 0 .. G-1:  for j = 0 .. J_g-1:  acc = acc + (R_g[k][j] s_g[b][j])
 *     v = (leak u[b][k]) - (gain acc);   stroke > 0:  v = v < -stroke ? -stroke : v;  v = v > stroke ? stroke : v;   u[b][k] = v
 * in float64, every product and every sum rounded on its own in that order (never a fused multiply-add): a host replay is bit-exact.
 * inputs_host: HOST array of G device pointers, s_g [B][J_g] float64.  out_u_dev [B][K] (nullable) receives u of every env as it stands
 * after the call (an env the mask leaves out keeps its u).  A small GEMM: a workgroup owns 32 envs x 64 outputs, stages 64 columns of the
 * envs' s and of its R rows in LDS at a time, and a thread carries one output of 8 envs; every R row is read once per env tile.  The
 * order of the sum of one (b, k) does not depend on the tiling: a split batch gives the bits of the whole.
 *
 * aog_tomo_reset zeroes u of the selected envs.  Every call is ordered by the one stream it is given; none waits for the device.
 * AOG_ERR_INVALID, before any device work, with aog_last_error naming the entry point and the field: a null handle, config or required
 * array; a wrong abi_version, num_envs < 1, n_out, n_inputs or a width outside its range, a width != 0 beyond n_inputs, env_id_base < 0,
 * reserved != 0; g outside 0 .. G-1; gain or leak not finite, stroke NaN. */
typedef struct aog_tomo aog_tomo;
typedef struct aog_tomo_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, n_out, n_inputs;
  int32_t width[4];
  int32_t env_id_base;
  int32_t reserved;                     /* 0 */
} aog_tomo_config;
int64_t aog_tomo_config_size(void);
int aog_tomo_create(const aog_tomo_config* cfg, int device, aog_tomo** out);
void aog_tomo_destroy(aog_tomo* tomo);
int aog_tomo_upload(aog_tomo* tomo, int g, const double* R_dev, void* stream);
int aog_tomo_update(aog_tomo* tomo, const double* const* inputs_host, double gain, double leak, double stroke, const uint8_t* mask_dev,
                    double* out_u_dev, void* stream);
int aog_tomo_reset(aog_tomo* tomo, const uint8_t* mask_dev, void* stream);
int64_t aog_tomo_state_bytes(const aog_tomo* tomo);
int aog_tomo_get_state(aog_tomo* tomo, void* blob_dev, void* stream);
int aog_tomo_set_state(aog_tomo* tomo, const void* blob_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_TOMOGRAPHY_H */
