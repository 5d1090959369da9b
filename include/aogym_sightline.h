/* Layer altitudes and off-axis sightlines of the layered atmosphere (additive in ABI 22; no counterpart in the reference).  A layer at
 * altitude h is seen displaced by h x angle between two lines of sight, so a front that looks along an angle reads every layer of a
 * meta-pupil larger than the pupil at a sub-pixel displacement of its own (aog_install_layer_sum_sightline).  Declared here and not in
 * aogym.h for the reason aogym_disturbance.h gives: the stream-coverage rule is held for this header from files of its own
 * (tests/test_sightline_cpu.py, tests/test_gpu_sightline.py).  No struct, constant or signature of aogym.h changes. */
#ifndef AOGYM_SIGHTLINE_H
#define AOGYM_SIGHTLINE_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aog_install_layer_sum_sightline: aog_install_layer_sum with another definition of the value at env b and aperture pixel (iy, ix), and
 * layers that may be larger than the front.
 *
 * Handles.  dst: a quasi-static front with pupil N, tables uploaded.  Layer l: a dynamic handle with screens, of N_l >= N pixels at the
 * same pixel pitch, N_l - N even; c_l = (N_l - N) / 2 is the margin of the meta-pupil on every side.  Device, B and env_id_base of every
 * layer are the front's.  n_layers in 1 .. 8.  A fast front must run the MFMA kernel (AOG_ERR_UNSUPPORTED on a VALU front).
 *
 * Shifts.  shift_host: a HOST array [n_layers][B][2] float64, (sx, sy) of layer l and env b in pixels.  Checked on the host before
 * anything is launched or changed: finite, and |sx|, |sy| <= c_l - 1 (exactly 0 when c_l = 0) — AOG_ERR_INVALID naming layer, env
 * and margin otherwise.  They are copied to a buffer the front owns, through pinned staging and on `stream`, and only when they differ
 * from the values of the front's last installation (the staging buffer keeps those); the caller's array is free when the call returns.
 *
 * The value.  With y0 = floor(sy), fy = sy - y0, gy = 1 - fy and x0, fx, gx likewise (each one rounded float64 operation, formed once
 * per env and layer), front pixel (iy, ix) of env b reads layer l at the logical position (iy + c_l + sy, ix + c_l + sx) bilinearly:
 *     v00 = layer_l[iy + c_l + y0    ][ix + c_l + x0    ]      v01 = layer_l[iy + c_l + y0    ][ix + c_l + x0 + 1]
 *     v10 = layer_l[iy + c_l + y0 + 1][ix + c_l + x0    ]      v11 = layer_l[iy + c_l + y0 + 1][ix + c_l + x0 + 1]
 *     v_l = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))
 * in float64, every product and every sum rounded on its own in the order the brackets give (never a fused multiply-add), so that a host
 * restatement is bit-exact.  With fx = fy = 0 this is v00.  layer_l[y][x] is the layer's logical screen (what aog_get_screens_f64
 * returns): the master ring read through the layer's own origin, physical row (y + oy) mod N_l and column (x + ox) mod N_l.  The kernels
 * fold c_l, the integer part and the origin into one offset per axis, env and layer, reduced modulo N_l, so every address lies inside the
 * layer's screen whatever the shift; the check above is what keeps a sample from wrapping round the ring into unrelated data.
 *     s = v_0 + v_1 + ... + v_{L-1}                                              (float64, layer order)
 *     s = s + coeff[b][0] basis[0][p];  ...;  s = s + coeff[b][K-1] basis[K-1][p]   (as aog_install_layer_sum_disturbed)
 * The aperture mean of THIS s is removed, in the fixed order aogym_disturbance.h states, and s - mean is written exactly as
 * aog_install_layer_sum writes it: psi_tile on fast MFMA fronts (pad pixels and pad envs exact zeros), psi64 on float64 fronts.  No
 * atomics; an env's result does not depend on the batch it sits in.
 *
 * Terms.  n_terms = 0: no modal terms, coeff_dev is not read (it may be null).  n_terms > 0: coeff_dev [B][n_terms] float64 on the
 * device, read on `stream`; the front must hold a basis of n_terms terms (aog_upload_disturbance_basis) — AOG_ERR_INVALID otherwise.
 *
 * Attenuation.  A bilinear read is exact at whole-pixel shifts (a translation) and attenuates the highest spatial frequencies at
 * fractional ones: per axis the amplitude at angular frequency w (radians per pixel) is multiplied by |(1 - f) + f exp(-i w)|, which at
 * half a pixel is cos(w / 2) — zero at the Nyquist frequency of the grid, 0.92 at a quarter of it.
 *
 * With N_l = N and all-zero shifts the front is left with the bits of aog_install_layer_sum (n_terms = 0) or of
 * aog_install_layer_sum_disturbed.  The other checks, the outputs and the stream order are aog_install_layer_sum's. */
int aog_install_layer_sum_sightline(aog_env* dst, aog_env* const* layers, int n_layers, const double* shift_host, const double* coeff_dev, int n_terms,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_SIGHTLINE_H */
