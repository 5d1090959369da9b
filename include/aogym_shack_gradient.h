/* The analytic gradient of the Shack-Hartmann chain: clean image, clean slopes and their vector-Jacobian product with respect to the mirror
 * (additive in ABI 22; no counterpart in the reference).  Declared here and not in aogym.h for the reason aogym_disturbance.h gives: the
 * stream-coverage rule is held for this header from files of its own (tests/test_shack_gradient_cpu.py, tests/test_gpu_shack_gradient.py).
 * No struct, constant or signature of aogym.h changes. */
#ifndef AOGYM_SHACK_GRADIENT_H
#define AOGYM_SHACK_GRADIENT_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aog_sh_gradient: the gradient of
 *     L = sum(g_image * image) + sum(g_slopes * slopes)
 * with respect to the actuators (metres of surface) of every env `mask_dev` selects (NULL: all), after aog_upload_sh.
 *
 * image [B][N*N] is the noise-free detector image of aog_sh_image; slopes [B][2 n_sub] are the centroids of image + 1e-10 over the
 * selected lenslets minus the lenslet centres and the reference slopes, all s_x then all s_y: what aog_sh_update's integrator multiplies
 * by the reconstructor, without photon noise.  g_image_dev [B][N*N] and g_slopes_dev [B][2 n_sub]: float64 device cotangents, either may
 * be NULL (zero).  act_dev [B][A] float64: the point of evaluation; NULL = the sensor's own mirror (deformable_mirror_shack.actuators, what
 * aog_sh_update integrates), which is never written.  grad_dev [B][A] float64.  image_dev / slopes_dev (nullable): the clean values at
 * that point.  grad_dev = NULL with both cotangents NULL runs the forward half alone.  The rows of the envs the mask leaves out are not
 * written in any output.
 *
 * The call draws no noise and leaves alone everything aog_sh_image / aog_sh_update and a step read or write later: the noise call
 * counter, the per-lenslet sums of a fused aog_sh_image call and their flag, the image a noise-drawing aog_sh_update call reads, the
 * integrator's actuators, the env's mirror and every step output.  Work buffers of its own are made by the first call.
 *
 * Routes.  Handles on the separable two-pass propagation (N = 128, 256, 512, 240, 480 in complex64 with a factorising transfer function)
 * run the forward passes of aog_sh_image as they stand (the image has aog_sh_image's bits) and two register-resident backward passes
 * with the conjugated transfer function; the modes contraction uses the operands of aog_upload_gradient; without them AOG_ERR_STATE.
 * Every other handle runs hipFFT on the padded 2N x 2N grid in the handle's transform precision.
 *
 * Refusals: aog_sh_image's own (before aog_upload_sh / aog_set_screens, a pending pipelined action, between two steps of a lookahead
 * episode), a poisoned handle, and AOG_ERR_INVALID for grad_dev = NULL with a cotangent, both cotangents NULL with grad_dev, or nothing to
 * write at all.  Stream-ordered on `stream`; no host synchronisation after the first call. */
int aog_sh_gradient(aog_env* env, const uint8_t* mask_dev, const double* g_image_dev, const double* g_slopes_dev, const double* act_dev,
                    double* grad_dev, double* image_dev, double* slopes_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_SHACK_GRADIENT_H */
