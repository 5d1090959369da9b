/* Modal disturbance on top of the layered atmosphere: vibration and static aberrations (additive in ABI 22; no counterpart in the
 * reference).  K <= 8 fixed pupil shapes; per env and shape a coefficient = a static offset + a stochastic vibration generated on the
 * device (aog_disturbance_*); the coefficients enter the layer sum a front handle installs (aog_install_layer_sum_disturbed).  Declared
 * here and not in aogym.h so that the rule tests/test_stream_coverage_cpu.py holds aogym.h to is held for this header from files of its
 * own (tests/test_disturbance_stream_coverage_cpu.py, tests/test_gpu_disturbance_streams.py).  No struct, constant or signature of
 * aogym.h changes. */
#ifndef AOGYM_DISTURBANCE_H
#define AOGYM_DISTURBANCE_H

#include "aogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AOG_DISTURBANCE_MAX_TERMS = 8 };

/* ---- the generator: a handle of its own, independent of any aog_env (as aog_spgd, aog_link) ----
 * Parameters per (env b, term k), float64, 0 until aog_disturbance_set_params: a1, a2, b (the AR(2) recursion), sigma, rho1 (its
 * stationary standard deviation and lag-1 correlation, for the start), offset (the static part).  State per (env, term): x, x_prev
 * (float64); per handle one 64-bit call counter c, which every aog_disturbance_reset and aog_disturbance_advance raises by 1 whatever
 * its mask.
 *
 *   Normals.  normal(b, k, j), j in {0, 1}, of the call that finds the counter at c is standard normal number
 *     idx = ((c mod 2^27) << 5) | (j << 3) | k   of the stream   (seed, env_id_base + b, 0xD1570000 + floor(c / 2^27))
 *   of philox_normal (csrc/k_common.h): element idx & 3 of the Philox4x32-10 call keyed by seed (low word, high word) with counter
 *   (idx >> 2, 0xD1570000 + floor(c / 2^27), env_id_base + b, 0).  An env's numbers depend on its GLOBAL id and on c alone, never on the
 *   batch it sits in: handles that hold the parts of a batch and receive the same calls reproduce the whole batch bit for bit.
 *
 *   aog_disturbance_reset, selected envs: n0 = normal(b, k, 0), n1 = normal(b, k, 1),
 *     x_prev = sigma n0,   x = sigma (rho1 n0 + sqrt(1 - rho1 rho1) n1)
 *   — the stationary start of the recursion.  noise_out: nullable [B][K][2] float64, receives (n0, n1) of the selected envs.
 *   aog_disturbance_advance, selected envs: n = normal(b, k, 0),
 *     x_new = (a1 x + a2 x_prev) + b n,   x_prev = x,   x = x_new,   coeff_out[b][k] = offset + x_new
 *   and noise_out [B][K] (nullable) receives n.  Envs the mask leaves out keep their state and get coeff_out[b][k] = offset + x; their
 *   entries of noise_out are not written.
 *   aog_disturbance_coefficients: coeff_out[b][k] = offset + x of every env; no state and no counter moves.
 *
 * Every product, sum and square root above is one rounded float64 operation in the order written (a1 x, then a2 x_prev, their sum,
 * b n, the sum; rho1 rho1, 1 - that, its root, rho1 n0, root n1, their sum, sigma times it); nothing is fused.  The root is formed once,
 * by aog_disturbance_set_params on the host (IEEE sqrt, correctly rounded).  A host replay from the recorded normals is therefore
 * bit-exact.  One thread per (env, term); plain vector stores, no atomics, no host synchronisation; the
 * calls on one handle are ordered by the one stream they are given.  mask_dev: nullable [B] uint8 device array, non-zero = selected.
 *
 * aog_disturbance_set_params: HOST arrays [B][K] each; a blocking copy that is not ordered behind any stream's pending calls.
 * AOG_ERR_INVALID, before any device work, with aog_last_error naming the entry point and the field: a wrong abi_version, num_envs < 1,
 * n_terms outside 1 .. 8; a non-finite parameter, sigma < 0, |rho1| > 1.  The struct is four int32 and a uint64 (24 bytes:
 * aog_disturbance_config_size); it has no index in aog_struct_size. */
typedef struct aog_disturbance aog_disturbance;
typedef struct aog_disturbance_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, n_terms, env_id_base;
  uint64_t seed;
} aog_disturbance_config;
int64_t aog_disturbance_config_size(void);
int aog_disturbance_create(const aog_disturbance_config* cfg, int device, aog_disturbance** out);
void aog_disturbance_destroy(aog_disturbance* gen);
int aog_disturbance_set_params(aog_disturbance* gen, const double* a1_host, const double* a2_host, const double* b_host, const double* sigma_host,
                               const double* rho1_host, const double* offset_host);
int aog_disturbance_reset(aog_disturbance* gen, const uint8_t* mask_dev, double* noise_out, void* stream);
int aog_disturbance_advance(aog_disturbance* gen, const uint8_t* mask_dev, double* coeff_out, double* noise_out, void* stream);
int aog_disturbance_coefficients(aog_disturbance* gen, double* coeff_out, void* stream);
/* Checkpointing: x [B][K], x_prev [B][K] (float64), then the counter (uint64): 16 B K + 8 bytes.  A handle of the same configuration and
 * parameters that takes the blob resumes bit-identically. */
int64_t aog_disturbance_state_bytes(const aog_disturbance* gen);
int aog_disturbance_get_state(aog_disturbance* gen, void* blob_dev, void* stream);
int aog_disturbance_set_state(aog_disturbance* gen, const void* blob_dev, void* stream);

/* ---- the installation ----
 * aog_upload_disturbance_basis: basis_host [n_terms][n_ap] float64, a HOST array — the pupil shapes at the aperture pixels in packed
 * aperture order (aog_tables.ap_index), in the unit of the master screens (hcipy's: phase * lambda = 2 pi x metres of optical path).
 * dst: tables uploaded, 1 <= n_terms <= 8, every value finite (AOG_ERR_INVALID otherwise).  A blocking copy; a second upload replaces
 * the first.
 *
 * aog_install_layer_sum_disturbed: aog_install_layer_sum with one other definition of the value at env b and aperture pixel p,
 *     s = master_0 + ... + master_{L-1}                                        (as aog_install_layer_sum: float64, layer order)
 *     s = s + coeff[b][0] basis[0][p];  ...;  s = s + coeff[b][K-1] basis[K-1][p]   (term order; each product rounded, then each sum)
 * The aperture mean of THIS s is removed and s - mean written exactly as aog_install_layer_sum writes it; the same checks, outputs,
 * stream order and batch independence.  The mean's fixed order (that of aog_install_layer_sum): 256 partial sums, partial t = s[t] +
 * s[t + 256] + s[t + 512] + ... ascending, from 0; each run of 64 consecutive partials folded in six halving steps (v[i] += v[i + off],
 * off = 32, 16, 8, 4, 2, 1); the four results added in order, from 0; the total divided by n_ap.  coeff_dev: [B][n_terms] float64 on the device (what aog_disturbance_advance writes), read on
 * `stream`.  In addition AOG_ERR_INVALID for a null coeff_dev, a dst without an uploaded basis, and an n_terms other than the uploaded
 * basis's.  All-zero coefficients leave the bits of aog_install_layer_sum. */
int aog_upload_disturbance_basis(aog_env* dst, const double* basis_host, int n_terms);
int aog_install_layer_sum_disturbed(aog_env* dst, aog_env* const* layers, int n_layers, const double* coeff_dev, int n_terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_DISTURBANCE_H */
