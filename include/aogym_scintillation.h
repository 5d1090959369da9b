/* Scintillation of the layered atmosphere (additive in ABI 22; no counterpart in the reference): weak-turbulence (Rytov) propagation of
 * every layer above the ground to the pupil, and a receiver that sees the resulting amplitude.  A layer's screen phi on the meta-pupil
 * becomes, in the Fourier domain,
 *     S = F^-1[cos(kappa^2 z / 2k) F phi]      the diffracted phase
 *     chi = F^-1[sin(kappa^2 z / 2k) F phi]    the log-amplitude
 * one complex inverse transform of (cos + i sin) F phi.  A handle of its own, aog_scint, holds the filter tables and per layer the two
 * float64 meta-pupil surfaces S - phi (the diffraction correction) and chi.  Declared here and not in aogym.h for the reason
 * aogym_disturbance.h gives.  No struct, constant or signature of aogym.h changes.
 *
 * Configuration: B = num_envs >= 1, M = n_pixels >= 2 (the side of the meta-pupil the filtered layers are drawn on), L = n_layers in
 * 0 .. 8 (the layers above the ground, in layer order; 0: a receiver only, which filters and installs nothing), n_fiber in 1 .. 4 receive modes, reserved = 0, scratch_bytes > 0 the byte budget
 * of the transform buffer.  The struct is six int32 and one int64 (32 bytes: aog_scint_config_size).
 *
 * Edges.  A screen is not periodic; the transform runs on the even (mirror) extension of the meta-pupil, E = 2 M pixels a side:
 * ext[y][x] = phi[y < M ? y : 2 M - 1 - y][x < M ? x : 2 M - 1 - x], which is continuous across every edge.  What the remaining kink in
 * the slope leaks into the footprint is kept out by a guard band, which is the caller's (the Python layer adds it to the margin).
 *
 * Buffers the handle owns.
 *   filter[l][fy][fx]   float64 [L][E][E][2] (cos, sin) of layer l at FFT frequency (fy, fx) (aog_scint_upload): a HOST-built table, never
 *                       evaluated with device transcendentals, so a host restatement multiplies by the very same numbers
 *   corr[l][b][p]       float64 [L][B][M M]: S_l - phi_l in the masters' unit, logical pixel order (a ring that has not turned)
 *   chi[l][b][p]        float64 [L][B][M M]: chi_l in the masters' unit (phase x lambda), likewise
 *   work                complex128 [chunk][E][E], chunk = min(B, scratch_bytes / (16 E E)) >= 1: it does not grow with B
 *   wmodes              float64 [n_ptiles 32][4][2]: the receive modes (aog_scint_upload_modes), zero rows for pad pixels and modes
 *
 * aog_scint_filter, per chunk of envs and per layer: pack (the mirror extension of the layer's logical screen, imaginary part 0), a
 * forward hipFFT Z2Z, the multiply by (cos + i sin), an inverse Z2Z, unpack: corr = Re / E^2 - phi (one rounded product, one rounded
 * difference), chi = Im / E^2.  `layers`: the L dynamic handles, each of M pixels and the handle's B and device.  hipFFT is not
 * reproducible bit for bit against another transform; it is against itself, and an env's transform does not depend on its batch.
 *
 * aog_scint_correction(l): layer l's correction as an aog_altmirror view (surface = corr[l], ring origin 0, n_pixels = M), owned by the
 * handle: hand it to aog_install_layer_sum_conjugate as one more source at the layer's own shift and the front's phase becomes
 * sum_l S_l.  The one bilinear read of the installation kernels reads it.
 *
 * aog_scint_install: chi_tile[b][p] = (float) ((chi_0 + chi_1 + ... at the front's shifts) / lambda_wfs), each chi_l read bilinearly
 * exactly as aog_install_layer_sum_sightline reads a layer (the same device function), summed in layer order, for every aperture pixel of
 * the fast front `front`; chi_tile_dev is float32 in psi_tile's packed order [Bp / 32][n_ptiles][4][64][4] (aog_scint_tile_floats
 * elements), pad pixels and pad envs exact zeros.  shift_host: HOST array [L][B][2], checked like a sightline installation's (and, whatever
 * the values, every read is reduced modulo M: no address leaves a surface); shift_dev: the same values on the device, which the kernel
 * reads — the caller keeps both, so that a step copies nothing.
 *
 * aog_scint_receive, per env of the fast front, with u the residual phase in revolutions exactly as aog_wavefront_truth forms it (screen
 * tile plus modes x actuators on the matrix cores), a = exp(chi) in float32 and sums in float64 over the aperture:
 *     c_k = sum_p W_k[p] a_p exp(2 pi i u_p)        power = sum_k |c_k|^2 (chi = 0: the step's power)
 *     irradiance = sum_p a_p^2 / n_ap
 *     strehl = |sum_p a_p exp(2 pi i u_p)|^2 / (sum_p a_p)^2
 *     sigma_chi2 = sum_p chi_p^2 / n_ap - (sum_p chi_p / n_ap)^2
 * each a float64 [B] device output.  chi_tile_dev may be null: chi = 0.  An env's sums depend on its own column alone and are added in a
 * fixed order: a batch split over two handles gives the bits of the whole batch.
 *
 * Every call is ordered by the one stream it is given; a handle is used on one stream at a time.  AOG_ERR_INVALID before any device
 * work for null arguments and mismatched sizes, AOG_ERR_UNSUPPORTED for a front that is not a fast MFMA handle. */
#ifndef AOGYM_SCINTILLATION_H
#define AOGYM_SCINTILLATION_H

#include "aogym_conjugate.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_SCINT_MAX_LAYERS = 8, AOG_SCINT_MAX_FIBER = 4 };

typedef struct aog_scint aog_scint;
typedef struct aog_scint_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, n_pixels, n_layers, n_fiber;
  int32_t reserved;                     /* 0 */
  int64_t scratch_bytes;
} aog_scint_config;
int64_t aog_scint_config_size(void);
int aog_scint_create(const aog_scint_config* cfg, int device, aog_scint** out);
void aog_scint_destroy(aog_scint* scint);
int aog_scint_upload(aog_scint* scint, const double* filter_dev, void* stream);
int aog_scint_upload_modes(aog_scint* scint, aog_env* front, const double* modes_host);
int aog_scint_filter(aog_scint* scint, aog_env* const* layers, void* stream);
aog_altmirror* aog_scint_correction(aog_scint* scint, int layer);
int aog_scint_get(aog_scint* scint, int layer, double* corr_out, double* chi_out, void* stream);
int64_t aog_scint_tile_floats(const aog_env* front);
int64_t aog_scint_scratch_bytes(const aog_scint* scint);
int aog_scint_install(aog_scint* scint, aog_env* front, const double* shift_host, const double* shift_dev, float* chi_tile_dev, void* stream);
int aog_scint_receive(aog_scint* scint, aog_env* front, const float* chi_tile_dev, double* power_dev, double* irradiance_dev, double* strehl_dev,
                      double* sigma_chi2_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_SCINTILLATION_H */
