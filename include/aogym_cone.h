/* Finite-range sources of the layered atmosphere: the cone effect (additive in ABI 22; no counterpart in the reference).  Light from a
 * source at range H — a laser guide star, an aircraft or satellite terminal — crosses a layer at altitude h inside a cone: its footprint on
 * the layer is the pupil shrunk by m = 1 - h / H about the point the line of sight crosses the layer at.  aog_install_layer_sum_cone is
 * aog_install_layer_sum_conjugate (aogym_conjugate.h) with that one more number per source and env.  Declared here and not in
 * aogym_sightline.h or aogym_conjugate.h for the reason aogym_disturbance.h gives: the stream-coverage rule is held for this header from
 * files of its own (tests/test_cone_cpu.py, tests/test_gpu_cone.py).  No struct, constant or signature of another header changes. */
#ifndef AOGYM_CONE_H
#define AOGYM_CONE_H

#include "aogym_conjugate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aog_install_layer_sum_cone: aog_install_layer_sum_conjugate with another position of the sample.
 *
 * Handles, counts, terms, outputs and stream order are that entry point's: dst a quasi-static front with pupil N; n_layers >= 1 dynamic
 * handles with screens, then n_mirrors >= 0 altitude mirrors (mirrors may be null when there are none), n_layers + n_mirrors <= 8; source
 * l has N_l >= N pixels, N_l - N even, margin c_l = (N_l - N) / 2; a mirror is read as a layer whose ring origin is 0.
 *
 * Geometry.  geom_host: a HOST array [n_layers + n_mirrors][B][3] float64, (sx, sy, m) of source l and env b, the layers' first: the
 * shift in pixels as aog_install_layer_sum_sightline's, and the magnification.  With ctr = (N - 1) / 2 (exact in float64), front pixel
 * (iy, ix) of env b reads source l at the logical position
 *     (c_l + ctr + m (iy - ctr) + sy,  c_l + ctr + m (ix - ctr) + sx)
 * bilinearly.  The position is formed as the sightline's, i + c_l + floor(s), plus a correction that is an exact zero at m = 1.  Per
 * axis, with i the pixel's index and s the shift on that axis, in float64, every operation rounded on its own, in this order and never a
 * fused multiply-add:
 *     s0 = floor(s), r = s - s0, k = m - 1      (once per env and source)
 *     e = k * (i - ctr)                           (i - ctr is an exact half-integer)
 *     q = e + r
 *     q0 = floor(q)
 *     f = q - q0
 *     g = 1 - f
 * and the first sample's index on that axis is i + s0 + q0 (s0 and q0 as integers): (y0, fy, gy) from (iy, sy) with y0 = iy + s0 + q0, and
 * (x0, fx, gx) from (ix, sx) likewise.  In exact arithmetic i + s0 + q + c_l is the position above.  At m = 1: k = 0, e = 0, q = r, q0 = 0,
 * f = s - floor(s) — the index and the weights of aogym_sightline.h to the bit, with no separate case.  (The order proposed first,
 * p = m (i - ctr) + (ctr + s) and f = p - floor(p), rounds the weight at the magnitude of the pixel index where s - floor(s) is rounded
 * at the magnitude of the shift; the two differ by up to N 2^-53, and an env at m = 1 would have held other bits in a batch routed here
 * than in one routed to the plane-wave entry points.)  Then
 *     v00 = src_l[c_l + y0    ][c_l + x0    ]      v01 = src_l[c_l + y0    ][c_l + x0 + 1]
 *     v10 = src_l[c_l + y0 + 1][c_l + x0    ]      v11 = src_l[c_l + y0 + 1][c_l + x0 + 1]
 *     v_l = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))
 * exactly as aogym_sightline.h brackets it; src_l[y][x] is the source's logical screen (the master ring read through the layer's own
 * origin; a mirror's surface as it stands), indices modulo N_l.  The kernels fold c_l and the origin into one offset per axis, env and
 * source; the check below keeps every sample inside the source's screen and away from the ring's wrap.
 *     s = v_0 + v_1 + ... + v_{L-1} + w_0 + ... + w_{n_mirrors-1}               (float64, source order)
 *     s = s + coeff[b][0] basis[0][p];  ...;  s = s + coeff[b][K-1] basis[K-1][p]   (as aog_install_layer_sum_disturbed)
 * The aperture mean of THIS s is removed, in the fixed order aogym_disturbance.h states, and s - mean is written exactly as
 * aog_install_layer_sum writes it: psi_tile on fast MFMA fronts (pad pixels and pad envs exact zeros), psi64 on float64 fronts.  No
 * atomics; an env's result does not depend on the batch it sits in.  A host restatement of this text is bit-exact.
 *
 * Checks, on the host before anything is launched or changed (aog_cone_check_geometry is the same code without the handles).
 * AOG_ERR_INVALID naming the source ("layer l" / "mirror j"), the env and the margin unless, for every source and env,
 *     sx, sy and m are finite,   0 < m <= 1,   and on each axis   |s| + (1 - m) (N - 1) / 2 <= c_l - 1
 * (one rounded difference, product, sum; with c_l = 0 this asks for s = 0 and m = 1 exactly).  The bound keeps the first sample at or
 * above logical index 1 and the second at or below N_l - 1.  The handle, size, device and n_terms checks are
 * aog_install_layer_sum_conjugate's.  The values are copied to a buffer the front owns through pinned staging on `stream`, and only when
 * they differ from those of the front's last installation; the caller's array is free when the call returns.
 *
 * m = 1.  With m = 1 for every source the front is left with the bits of aog_install_layer_sum_conjugate, at whole-pixel and at
 * fractional shifts: every index and weight is the sightline form's, as said above.  An env of a mixed batch whose sources all have m = 1
 * holds those bits too, so a caller may send plane-wave envs through either entry point.
 *
 * Not modelled: the amplitude of a spherical wave, the elongation of a laser spot, and focus or tilt indetermination (those are the
 * caller's to impose on what is measured). */
int aog_install_layer_sum_cone(aog_env* dst, aog_env* const* layers, int n_layers, aog_altmirror* const* mirrors, int n_mirrors,
                               const double* geom_host, const double* coeff_dev, int n_terms, void* stream);

/* aog_cone_check_geometry: the geometry check of aog_install_layer_sum_cone alone, for a caller that wants to refuse a geometry before
 * it has handles: geom_host as above for num_envs = B envs, a front of n_pupil = N pixels and source_pixels[l] = N_l.  No device, no
 * handle, no stream.  AOG_OK, or AOG_ERR_INVALID with aog_last_error as the installation words it: null arrays, n_layers < 1,
 * n_mirrors < 0, more than 8 sources, num_envs < 1, n_pupil < 1, N_l < N or N_l - N odd, and the three checks above. */
int aog_cone_check_geometry(const double* geom_host, int n_layers, int n_mirrors, int num_envs, int n_pupil, const int32_t* source_pixels);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_CONE_H */
