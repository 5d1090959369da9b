/* Altitude-conjugated deformable mirrors of the layered atmosphere (additive in ABI 22; no counterpart in the reference).  A mirror
 * conjugated to an altitude h is seen displaced by h x angle between two lines of sight, exactly as a turbulent layer at h is: its
 * surface lives on the meta-pupil, and every front reads the footprint its own angle selects.  A handle of its own, aog_altmirror, turns a
 * command into that surface (and a layer's screen into its best-fit command); aog_install_layer_sum_conjugate reads such surfaces beside
 * the layers.  Declared here and not in aogym.h for the reason aogym_disturbance.h gives: the stream-coverage rule is held for this header
 * from files of its own (tests/test_conjugate_cpu.py, tests/test_gpu_conjugate.py).  No struct, constant or signature of aogym.h changes. */
#ifndef AOGYM_CONJUGATE_H
#define AOGYM_CONJUGATE_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_ALTMIRROR_MAX_MODES = 256 };

/* Configuration: B = num_envs >= 1, M = n_pixels >= 1 (the side of the square grid the surface is drawn on: the meta-pupil's, or the
 * pupil's for a mirror at altitude 0), K = n_modes in 1 .. 256, reserved = 0; B M M must stay below 2^31.  There is no random stream and
 * therefore no seed and no env id.  The struct is five int32 (20 bytes: aog_altmirror_config_size); it has no index in aog_struct_size.
 *
 * Buffers the handle owns.
 *   basis[k][p]     float64 [K][M M]: the surface per unit command of mode k (aog_altmirror_upload); zeros until the first upload
 *   fit[k][p]       float64 [K][M M], optional: the matrix of aog_altmirror_fit
 *   command[b][k]   float64 [B][K]: the record, and the checkpoint blob; zero at creation
 *   surface[b][p]   float64 [B][M M]; zero at creation
 *   origin[b]       int32 [B][2], all zero: a surface is read as a layer whose ring has not turned
 *
 * Units.  The unit of the surface is the unit of the master screens (aogym_disturbance.h: phase x lambda = 2 pi x metres of optical
 * path).  A basis row is that per unit command; what a unit command means is the caller's choice (the Python layer makes it one metre of
 * optical path at an influence function's peak).
 *
 * aog_altmirror_upload copies the DEVICE arrays basis_dev [K][M M] and fit_dev (nullable: the handle then has no fit, and loses one it
 * had) on `stream`.  The surfaces are not synthesised again: they follow the next aog_altmirror_set_command / aog_altmirror_set_state.
 *
 * aog_altmirror_set_command, for every env b the mask selects (mask_dev: nullable [B] uint8 device array, non-zero = selected):
 *   command[b][k] = cmd[b][k] for every k, exact copies, and for every p
 *     s = cmd[b][0] basis[0][p];  s = s + (cmd[b][1] basis[1][p]);  ...;  s = s + (cmd[b][K-1] basis[K-1][p]);  surface[b][p] = s
 * in float64, every product and every sum rounded on its own in that order (never a fused multiply-add, never a matrix instruction), so
 * that a host restatement is bit-exact.  An env the mask leaves out keeps command and surface bit for bit.  One launch; a lane holds one
 * pixel pair of 8 envs in registers, so a basis value it loads serves 8 envs; an env's commands are wave-uniform scalar loads; every
 * store is part of a whole coalesced row.  No atomics, no LDS: an env's surface depends on its own command and the basis alone, not on
 * the batch it sits in or on the mask.  cmd_dev must not be the handle's own record.
 *
 * aog_altmirror_get copies the record to cmd_out [B][K] and the surfaces to surface_out [B][M M] (each nullable) on `stream`.
 *
 * aog_altmirror_fit: cmd_out[b][k] = sum_p fit[k][p] screen_b[p] over the LOGICAL screen of `layer` — a dynamic aog_env with screens, of
 * N = M pixels and the mirror's B and device; screen_b[y][x] is what aog_get_screens_f64 returns, the master ring read through the
 * env's origin.  float64; per-thread strided sums, then a fixed tree over the workgroup: no atomics, and an env's result is the same bits
 * in any batch.  It is a sum of M M terms in some fixed order: |error| <= M M 2^-53 sum_p |fit[k][p] screen_b[p]|.  `fit` is the caller's
 * matrix (the pseudo-inverse of the basis gives the least-squares command; minus that command cancels the layer as well as the mirror
 * can).  AOG_ERR_INVALID when no fit was uploaded, when the layer is not such a handle or when sizes or device differ.
 *
 * State.  aog_altmirror_get_state copies command [B][K] float64 (8 B K bytes); aog_altmirror_set_state copies the commands in and
 * synthesises every env's surface again on `stream`, so a restored mirror is complete without a further call (the basis is not part of
 * the state: upload it first).
 *
 * Every call is ordered by the one stream it is given; none waits for the device.  AOG_ERR_INVALID, before any device work, with
 * aog_last_error naming the entry point and the field: a null handle, config, output or required array; a wrong abi_version,
 * num_envs < 1, n_pixels < 1 (or B M M >= 2^31), n_modes outside 1 .. 256, reserved != 0. */
typedef struct aog_altmirror aog_altmirror;
typedef struct aog_altmirror_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, n_pixels, n_modes;
  int32_t reserved;                     /* 0 */
} aog_altmirror_config;
int64_t aog_altmirror_config_size(void);
int aog_altmirror_create(const aog_altmirror_config* cfg, int device, aog_altmirror** out);
void aog_altmirror_destroy(aog_altmirror* mirror);
int aog_altmirror_upload(aog_altmirror* mirror, const double* basis_dev, const double* fit_dev, void* stream);
int aog_altmirror_set_command(aog_altmirror* mirror, const double* cmd_dev, const uint8_t* mask_dev, void* stream);
int aog_altmirror_get(aog_altmirror* mirror, double* cmd_out, double* surface_out, void* stream);
int aog_altmirror_fit(aog_altmirror* mirror, aog_env* layer, double* cmd_out, void* stream);
int64_t aog_altmirror_state_bytes(const aog_altmirror* mirror);
int aog_altmirror_get_state(aog_altmirror* mirror, void* blob_dev, void* stream);
int aog_altmirror_set_state(aog_altmirror* mirror, const void* blob_dev, void* stream);

/* aog_install_layer_sum_conjugate: aog_install_layer_sum_sightline (aogym_sightline.h) with n_mirrors further sources after the layers,
 * in the order given.  Mirror j is read exactly as a layer of N_l = M_j pixels: margin c = (M_j - N) / 2 (M_j >= N, the difference even),
 * ring origin 0, screen = its surface, bilinearly at its own shift; it is added with a plus sign, in source order, inside the same
 * float64 sum:
 *     s = v_0 + ... + v_{L-1} + w_0 + ... + w_{n_mirrors-1}
 * then the modal terms, the mean and the stores as aog_install_layer_sum_sightline's.  n_layers >= 1, n_mirrors >= 0 (mirrors may be null
 * then), n_layers + n_mirrors <= 8.  shift_host: HOST array [n_layers + n_mirrors][B][2], the layers' shifts first; every source's shifts
 * pass the same margin check, the message naming "layer l" or "mirror j".  Every mirror has the front's B and device.  It runs the
 * kernels of aog_install_layer_sum_sightline at n_layers + n_mirrors sources; with n_mirrors = 0 the front is left with that entry
 * point's bits.  The surfaces are read on `stream`: behind an aog_altmirror_set_command made on the same stream. */
int aog_install_layer_sum_conjugate(aog_env* dst, aog_env* const* layers, int n_layers, aog_altmirror* const* mirrors, int n_mirrors,
                                    const double* shift_host, const double* coeff_dev, int n_terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_CONJUGATE_H */
