/*
 * aogym.h — C-ABI of libaogym.so: the MI355X (gfx950) implementation of the AOEnv.step() hot path.
 *
 * The reference (payamparvizi/adaptive_optics_gym) is pure Python on top of hcipy; it has no FFI.
 * The interface each entry point replaces is therefore a *Python* call site in
 * gym_AO/envs/AO_env.py (cited per function).  The reference-side binding a maintainer would add is
 * a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success or a negative aog_status; it never throws, never exits;
 *     aog_last_error() returns a thread-local message for the last failure on this thread.
 *   - pointers named *_dev are device pointers owned by the CALLER (e.g. torch tensors); the library
 *     owns only the handle, its constant tables and its per-environment state.
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered and asynchronous.
 *   - one handle per device; a handle is not thread-safe; distinct handles are independent.
 *   - there is no CPU fallback: creating a handle without a HIP device fails with AOG_ERR_HIP.
 */
#ifndef AOGYM_H
#define AOGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOG_ABI_VERSION 22

typedef struct aog_env aog_env;

typedef enum {
  AOG_OK = 0,
  AOG_ERR_INVALID = -1,     /* bad argument / unsupported configuration              */
  AOG_ERR_HIP = -2,         /* a HIP runtime call failed (message has the HIP error) */
  AOG_ERR_STATE = -3,       /* call order violated (e.g. step before upload_tables)  */
  AOG_ERR_UNSUPPORTED = -4  /* valid in the reference, not built yet                 */
} aog_status;

enum { AOG_REWARD_STREHL = 0, AOG_REWARD_SMF_SSIM = 1 };           /* AO_env.py:476,487 */
enum { AOG_PRECISION_FAST = 0, AOG_PRECISION_FP64 = 1 };           /* fp32 data / fp64 validation kernel */
enum { AOG_KERNEL_AUTO = 0, AOG_KERNEL_VALU = 1, AOG_KERNEL_MFMA = 2 };

/* Scalar configuration.  Mirrors AOEnv.__init__ kwargs (AO_env.py:17-29) and the constants fixed by
 * parameters_init (AO_env.py:211-247) that the device path consumes. */
typedef struct {
  int32_t abi_version;          /* = AOG_ABI_VERSION                                            */
  int32_t num_envs;             /* B: environments stepped in lock-step                         */
  int32_t n_pupil;              /* N: pupil grid side (reference: 240, AO_env.py:216)            */
  int32_t n_modes;              /* A = act_dim (AO_env.py:223)                                   */
  int32_t obs_dim;              /* o (AO_env.py:236)                                             */
  int32_t n_ap;                 /* aperture pixels (packed list length)                          */
  int32_t n_wfs_tables;         /* real pupil-plane tables at lambda_wfs                         */
  int32_t n_sci_tables;         /* real pupil-plane tables at lambda_sci                         */
  int32_t n_fiber_modes;        /* guided LP modes (3 at V = 2.639)                              */
  int32_t reward_type;          /* AOG_REWARD_*                                                  */
  int32_t sh_operation;         /* 1: action = raw actuators (AO_env.py:115-116)                 */
  int32_t max_steps;            /* timesteps_per_episode (AO_env.py:227)                         */
  int32_t flat_mirror_start;    /* flat_mirror_start_per_episode (AO_env.py:79-80)               */
  int32_t has_rew_threshold;    /* rew_threshold is not None (AO_env.py:500)                     */
  int32_t precision;            /* AOG_PRECISION_*                                               */
  int32_t kernel;               /* AOG_KERNEL_* (fast precision only)                            */
  int32_t pixel_chunks;         /* 0 = auto; number of pixel chunks the fused kernel splits into */
  int32_t atm_dynamic;          /* 1: atm_type == 'dynamic' (float64 master screens + wind extrusion each step) */
  int32_t env_id_base;          /* global id of this handle's env 0 (multi-GPU: rank r of a batch sharded contiguously owns
                                   envs [env_id_base, env_id_base + num_envs)).  Every device random stream — screen synthesis,
                                   extrusion normals, Shack-Hartmann photon noise — is keyed by the GLOBAL env id, so results do
                                   not depend on how the batch is split over handles / GPUs              */
  int32_t obs_separable;        /* observation route (ABI 20).  0: the o^2 observation pixels are pupil-plane kernels in wfs_tables /
                                   wfs_coef (fast handles o <= 5, float64 handles o <= 8).  1: wfs_tables / wfs_coef describe the fiber
                                   modes only and the observation is the separable matrix Fourier transform obs = |M1 (A o E) M2|^2
                                   uploaded by aog_upload_obs_mft (any o <= 32; the policy kernel's state_dim <= 1024 sets the limit)    */
  double wavelength_wfs;        /* 1.5e-6 (AO_env.py:219)                                        */
  double wavelength_sci;        /* 2.2e-6 (AO_env.py:220)                                        */
  double surface_rms_target;    /* 0.1*wavelength_sci (AO_env.py:120)                            */
  double rew_threshold;         /* used iff has_rew_threshold                                    */
  double ssim_ref_peak;         /* 2.8 (AO_env.py:492)                                           */
  double ssim_alpha;            /* 0.8 (AO_env.py:497)                                           */
} aog_config;

/* Host-precomputed constant tables (float64, HOST pointers; copied and converted by the call).
 * They are what AOEnv.__init__ precomputes through hcipy (AO_env.py:42-68, 293-393).
 *
 *   field at lambda_wfs on packed aperture pixel p:  E_p = exp(i*phi_p)  (amplitude folded into tables)
 *   U_m = sum_p cos(phi_p) g_m(p),  V_m = sum_p sin(phi_p) g_m(p)        (g = wfs_tables / sci_tables)
 *   Z_j = sum_m coef[j][m] * (U_m + i V_m)
 *   obs_raw[j] = |Z_j|^2  (j < o^2);  power = sum_k |Z_{o^2+k}|^2  (k < n_fiber_modes);
 *   strehl = |Z_sci|^2.
 * On the separable observation route (cfg.obs_separable = 1) the rows of wfs_coef are the fiber modes only (power = sum_k |Z_k|^2) and the
 * observation comes from aog_upload_obs_mft's matrices.
 */
typedef struct {
  const int32_t* ap_index;   /* [n_ap]  flat pupil index iy*N+ix of packed pixel p (row-major order) */
  const double* modes;       /* [n_ap][n_modes]  DM mode matrix restricted to the aperture (metres of
                                surface per unit actuator; AO_env.py:346-347,352-353)               */
  const double* gram;        /* [n_modes][n_modes]  centred Gram matrix: std_grid(M a)^2 = a' G a     */
  const double* wfs_tables;  /* [n_wfs_tables][n_ap]                                                 */
  const double* sci_tables;  /* [n_sci_tables][n_ap]                                                 */
  const double* wfs_coef;    /* [o^2 + n_fiber_modes][n_wfs_tables][2]  (re, im)                     */
  const double* sci_coef;    /* [1][n_sci_tables][2]                                                 */
  /* optional (NULL = aog_focal_image unsupported): the two matrices of the Fraunhofer matrix Fourier transform onto
   * the n_focal x n_focal fiber focal grid (propagator_fiber, AO_env.py:390), scale factors folded into focal_m1:
   *   F = focal_m1 [n_focal][N] . E [N][N] . focal_m2 [N][n_focal]                                           */
  const double* focal_m1;    /* [n_focal][N][2]                                                        */
  const double* focal_m2;    /* [N][n_focal][2]                                                        */
  int32_t n_focal;           /* 128 (AO_env.py:235)                                                    */
} aog_tables;

typedef struct {
  int32_t abi_version, num_envs, num_envs_padded, n_ap, n_ap_padded, n_modes_padded;
  int32_t pixel_chunks, kernel, n_sums;
  int32_t reserved;          /* flags: bit 0 = the dynamic atmosphere is read ring-direct, bit 1 = separable observation route */
  int64_t device_bytes;      /* bytes of HBM the handle owns */
} aog_info;

int aog_abi_version(void);
/* Identity of the sources this binary was compiled from: the first 32 hex digits of the SHA-256 over every csrc/ header and .hip file and this header
 * (adaptive_optics_gym_amd/build.py::source_id), "+FLAG" appended for developer builds.  The ctypes binding refuses a library whose id
 * differs from the sources it finds beside it. */
const char* aog_build_id(void);
const char* aog_last_error(void);
/* sizeof() of the structs of this header as the library was compiled, so that a binding in another language can verify its own
 * declarations at load time: which = 0 aog_config, 1 aog_tables, 2 aog_layer_tables, 3 aog_sh_tables, 4 aog_actor, 5 aog_info, 6 aog_layer_composite,
 * 7 aog_obs_mft, 8 aog_action_noise; -1 for any other value. */
int64_t aog_struct_size(int which);

/* AOEnv.__init__ (AO_env.py:17-71): allocate the handle and its state on `device`. */
int aog_create(const aog_config* cfg, int device, aog_env** out);
void aog_destroy(aog_env* env);
int aog_get_info(const aog_env* env, aog_info* out);

/* The part of AOEnv.__init__ that goes through hcipy (pupil_simulation, incoming_wavefront,
 * DM_function, fiber_coupling; AO_env.py:50-64). */
int aog_upload_tables(aog_env* env, const aog_tables* tables);

/* Separable observation route (cfg.obs_separable = 1; ABI 20): the two matrices of the Fraunhofer matrix Fourier transform onto the o x o
 * observation grid (propagator_fiber_subsample, AO_env.py:385,391), the observation scale folded into m1:
 *   obs_raw[v * o + u] = |sum_{y,x} m1[v][y] A[y][x] E[y][x] m2[x][u]|^2,   E = exp(i phi) on the pupil grid, A = aperture.
 * HOST pointers, float64, interleaved (re, im); converted once into the operand tables of the kernels.  aog_reset / aog_step on a separable
 * handle before this call return AOG_ERR_STATE. */
typedef struct {
  int32_t o;                 /* = cfg.obs_dim                                                        */
  int32_t reserved0;         /* = 0                                                                  */
  const double* m1;          /* [o][N][2]                                                            */
  const double* m2;          /* [N][o][2]                                                            */
} aog_obs_mft;
int aog_upload_obs_mft(aog_env* env, const aog_obs_mft* mft);

/* layer._achromatic_screen for envs [first, first+count) (hcipy InfiniteAtmosphericLayer state created at
 * AO_env.py:370 / regenerated at AO_env.py:77).  psi_dev: [count][N][N] achromatic screens (phase * lambda,
 * hcipy's unit), float64 or float32, row-major with x fastest.  The aperture mean of every screen is
 * removed (all outputs are invariant to a global phase) before conversion to the internal fp32 layout. */
int aog_set_screens_f64(aog_env* env, const double* psi_dev, int first, int count, void* stream);
int aog_set_screens_f32(aog_env* env, const float* psi_dev, int first, int count, void* stream);

/* hcipy InfiniteAtmosphericLayer construction products (AO_env.py:370; hcipy _make_stencils / _make_AB_matrices):
 * stencil positions and the auto-regressive extrusion matrices, shared by every env of the handle.  HOST pointers. */
typedef struct {
  int32_t nz_vertical, nz_horizontal;   /* stencil sizes (3N unless samples coincide)                        */
  const int32_t* stencil_vertical;      /* [nz_v] flat logical index iy*N+ix, increasing ('bottom' stencil)  */
  const int32_t* stencil_horizontal;    /* [nz_h] ('left' stencil)                                           */
  const double* A_vertical;             /* [N][nz_v]  new row    = A z + sqrt(Cn^2) B n                      */
  const double* B_vertical;             /* [N][N]                                                            */
  const double* A_horizontal;           /* [N][nz_h]  new column                                             */
  const double* B_horizontal;           /* [N][N]                                                            */
  double sqrt_cn_squared;               /* sqrt of AO_env.py:367                                             */
  double pixel_pitch;                   /* pupil_grid.delta (m)                                              */
  double delta_t;                       /* 1e-3 s (AO_env.py:226)                                            */
} aog_layer_tables;
int aog_upload_layer(aog_env* env, const aog_layer_tables* layer);

/* k_max successive one-pixel extrusions along one axis composed into ONE linear operator (exact: the same samples given the same normals;
 * adaptive_optics_gym_amd/extrusion_host.py::compose_extrusions builds it from the tables above):
 *     [R_1; ...; R_k] = A z_old + sqrt(Cn^2) B [n_1; ...; n_k],   R_j = the slice shift j of a step creates,
 * z_old = the screen BEFORE the first shift at the union of every sample the k stencils reach.  With both axes uploaded (after
 * aog_upload_layer, same k_max) aog_step advances a dynamic atmosphere with two matrix products per step on the int8 matrix cores
 * (csrc/k_extrude_i8.h: operands in base-128 digits, exact int32 accumulation; new samples good to ~1e-9 rad) instead of the chain of
 * one-pixel float64 rounds; operators for k < k_max are cut out of the uploaded one.  k_max must cover the largest whole-pixel shift any
 * env makes per step (floor(max wind component * delta_t / pixel_pitch) + 1) and be <= 8; steps the operators do not cover, float64
 * validation handles and AOG_EXTRUDE_F64 keep the float64 kernels.  HOST pointers.
 * Work ahead: what step t + 1 needs that depends on the clock, the winds and the screens step t's extrusion left — its shift plan and its
 * whole x phase, which writes operands and staged columns only — is launched by aog_step(t) on a low-priority stream of the library's own
 * and runs beside step t's remaining kernels and the caller's work between the two steps.  Invisible to the caller: every call that
 * changes what it read drops it, normals supplied for the next step redo it, results are bit for bit those of the in-line order
 * (AOG_X8_NO_PLAN_AHEAD=1 in the environment runs everything in line; AOG_X8_NO_PHASE_AHEAD=1 only the x phase). */
typedef struct {
  int32_t axis;             /* 0: vertical ('bottom' / 'top': new rows), 1: horizontal ('left' / 'right': new columns)             */
  int32_t k_max;            /* shifts composed                                                                                    */
  int32_t n_old;            /* U: size of the union stencil                                                                       */
  int32_t reserved0;
  const int32_t* old_yx;    /* [U] (sy << 16 | sx): logical position on the screen hcipy's _extrude sees, before the first shift   */
  const double* A;          /* [k_max N][U]: row (j - 1) N + i = sample i of the slice shift j creates                            */
  const double* B;          /* [k_max N][k_max N]: column (j' - 1) N + i' = normal i' of shift j' (without the sqrt(Cn^2) factor)  */
} aog_layer_composite;
int aog_upload_layer_composite(aog_env* env, const aog_layer_composite* op);
enum { AOG_EXTRUDE_AUTO = 0, AOG_EXTRUDE_F64 = 1 };   /* AUTO: the int8 composite form whenever its operators cover the step        */
int aog_set_extrusion_mode(aog_env* env, int mode);

/* layer.velocity of every env: [B][2] float64 (vx, vy) in m/s (hcipy draws the direction at construction).
 * max_abs_component >= max over envs of max(|vx|, |vy|): bounds the whole-pixel shifts per step.
 * Reads the velocities back once to group envs of similar wind for the extrusion kernel: synchronises `stream`. */
int aog_set_wind(aog_env* env, const double* velocity_dev, double max_abs_component, void* stream);

/* Lookahead for rollouts over a dynamic atmosphere.  The wind shift of step t + 1 (layer.t = ..., AO_env.py:125) depends on nothing
 * step t computes — only the product of the field with the evolved screen does (AO_env.py:132).  With lookahead on, aog_step(t) launches
 * the extrusion of step t + 1 on a stream of the library's own as soon as its fused kernel has finished reading the screens; it then runs
 * beside the step's epilogue and beside whatever the caller enqueues before aog_step(t + 1) (its policy query), and aog_step(t + 1) joins it.
 * Results are bit-identical with and without (same kernels, same random streams).  What changes: between the two calls the handle's screens
 * already stand at step t + 1, so aog_reset, aog_get_screens_f64, aog_get_state, aog_set_screens_*, aog_get_phase_screen, aog_focal_image(s)
 * and aog_sh_image return AOG_ERR_STATE there.  The last step of a lock-step episode (cfg.max_steps steps after the last whole-batch aog_reset)
 * never looks ahead, so all of them are available at episode boundaries — where a rollout calls them.  Needs the device random stream
 * (supplying normals with aog_set_extrusion_noise switches lookahead off for that step).  Off by default. */
int aog_set_lookahead(aog_env* env, int enable);

/* Standard normals for the extrusions of the NEXT aog_step: [B][max_ext][N] float64, consumed in hcipy's order (x shifts
 * first, then y).  NULL (default) = on-device Philox4x32-10 stream seeded by aog_set_rng_seed. */
int aog_set_extrusion_noise(aog_env* env, const double* noise_dev, int max_ext, void* stream);
int aog_set_rng_seed(aog_env* env, uint64_t seed);

/* Layered atmosphere: several frozen-flow layers per env, each an ordinary dynamic handle, summed into a quasi-static FRONT handle that
 * steps with the static fused kernel (on axis and conjugated to the pupil, L layers are exactly the sum of L independent screens).
 *
 * aog_evolve_atmosphere: the atmosphere half of aog_step and nothing else — timestep += 1, steps_since_reset += 1 and the wind extrusion
 * to that timestep; normals handed over with aog_set_extrusion_noise are consumed exactly as a step consumes them.  After k calls the
 * screens are bit for bit those of a twin that made k aog_step calls (the extrusion never reads the action).  AOG_ERR_STATE on a handle
 * that is not atm_dynamic, has no layer or screens, has lookahead on, whose atmosphere already stands at the next step, that has an action
 * pending or is poisoned; a failure after the counters moved poisons the handle as a failed aog_step does.
 *
 * aog_install_layer_sum: for env b and aperture pixel p, s = sum over l of master_l[b][(p + origin_l[b]) mod N] in float64 and in layer
 * order (each layer read through its own ring origin, each axis wrapping on its own); the aperture mean of s, summed in a fixed order,
 * is removed and float((s - mean) / (2 pi lambda_wfs)) is written into dst's fp32 screen tiles (MFMA accumulator order; pad pixels and
 * pad envs exactly 0); float64 validation handles get s - mean in their float64 screens.  dst: not atm_dynamic, tables uploaded
 * (AOG_ERR_INVALID otherwise; AOG_ERR_UNSUPPORTED on a handle that runs the VALU kernel); layers: 1 .. 8 dynamic handles with screens,
 * on dst's device, with dst's n_pupil, num_envs and env_id_base (AOG_ERR_INVALID otherwise).  A screen installation: on success dst has
 * screens and its kept reset observation is dropped; actuators, counters and the observation count stay, and an action a pipelined or
 * policy-attached step left pending stays pending.  Stream-ordered on `stream` (which must be the stream the layers evolve on), no host
 * synchronisation, no atomics; an env's output depends on that env's data only, so two handles of B / 2 reproduce one of B bit for bit.
 * The [B] float64 work buffer of the means is allocated by dst's first call. */
int aog_evolve_atmosphere(aog_env* env, void* stream);
int aog_install_layer_sum(aog_env* dst, aog_env* const* layers, int n_layers, void* stream);

/* layer._achromatic_screen of envs [first, first + count) as plain [count][N][N] float64 (hcipy's unit: phase * lambda).  Dynamic
 * handles return their float64 master screens; quasi_static / semi_dynamic handles return the stored screen exactly as the step
 * kernels read it: aperture pixels only (0 outside), aperture mean removed, fp32 values widened without rounding. */
int aog_get_screens_f64(aog_env* env, double* psi_dev, int first, int count, void* stream);

/* layer.reset() / layer construction (AO_env.py:77, :370): synthesise new von Karman screens for envs [first, first+count) ON THE
 * DEVICE and install them — hcipy's FiniteAtmosphericLayer + SpectralNoiseFactoryFFT: complex normals on the (oversampling N)^2
 * FFT grid times sqrt(PSD (2 pi)^2 / du^2), inverse FFT (hipFFT/rocFFT), real part of the central N x N crop / delta^2 * sqrt(Cn^2).
 * Normals come from the handle's Philox stream (aog_set_rng_seed); statistically equivalent to hcipy, not draw-for-draw: only the
 * half plane of spectrum lines 0..m/2 is drawn (a conjugate pair of independent complex normals with equal amplitudes contributes
 * to the REAL part exactly like one normal of sqrt(2) x the amplitude), and pupils of 64 R / 60 R pixels never materialise the
 * oversampled array (pruned two-pass transform). */
int aog_generate_screens(aog_env* env, int first, int count, int oversampling, double cn_squared, double outer_scale,
                         double pixel_pitch, void* stream);

/* Per-env turbulence strength (ABI 22): Cn^2 of every env, [B] float64 HOST values > 0 (AO_env.py:367 of each env's Fried parameter).
 * While they are set, aog_generate_screens draws env e at Cn^2_e (its cn_squared argument is only validated) and the wind extrusion of a
 * dynamic atmosphere adds sqrt(Cn^2_e) B n to env e's new samples: the float64 kernels read sqrt(Cn^2_e); the int8 tables keep the
 * aog_layer_tables.sqrt_cn_squared they were made at and env e's normals are scaled by c_e = sqrt(Cn^2_e) / sqrt_cn_squared before they are
 * digitised, so the layer must be uploaded at the batch's LARGEST Cn^2 (c_e <= 1; AOG_ERR_INVALID otherwise, here and in aog_upload_layer).
 * Every derived value is computed with the host arithmetic of the handle-wide value (aog_turbulence_factors): env e of a mixed batch gets
 * the bits of a uniform handle at Cn^2_e (int8 extrusion: envs with c_e = 1).  The library derives its per-env device arrays here and in
 * the first aog_generate_screens after a change (pinned staging, stream-ordered copies on `stream`); later calls copy nothing.
 * NULL returns the handle to the handle-wide value (today's code and bits).  Drops the int8 extrusion's work ahead; AOG_ERR_STATE between
 * two steps of a lookahead episode. */
int aog_set_turbulence(aog_env* env, const double* cn_squared_host, void* stream);

/* Photodetector model of the observations: shot noise, read noise and a calibrated background, per env ([B] float64 HOST arrays, copied
 * through pinned staging on `stream`).  With c_j = double(float(w_j)) the value a handle without a detector writes to obs_raw for pixel j,
 *   lam_j = photons_e c_j + background_e,   n_j = large_poisson(lam_j),   y_j = (n_j + read_noise_e g_j - background_e) / photons_e,
 *   obs_raw = float(y_j), obs = half(y_j)       (float64, no fused multiply-add; g_j standard normal)
 * photons: expected photo-electrons per frame of the whole unit-power beam (finite, > 0); read_noise: electrons rms per pixel and frame
 * (>= 0); background: electrons per pixel and frame (>= 0), subtracted again as a calibrated detector does.  AOG_ERR_INVALID otherwise.
 * ONLY THE OBSERVATION IS NOISY: reward (Strehl, and the SSIM term, which keeps reading the clean float64 powers), power, Strehl, done,
 * the return accumulator, screens and mirror are those of the handle without a detector bit for bit — the reward is the training signal of
 * the true state.  The fused tail (aog_reset_act / aog_step_act) feeds the policy the float16 that was stored.
 * Random stream: one Philox4x32-10 call per (global env, pixel, frame), key = the handle's rng_seed, counter = {j | 6 << 24,
 * env_id_base + e, frame & 0xFFFFFFFF, (frame >> 32) ^ 0xDE7EC7}; word 0 the Poisson uniform (radius of the rounded-normal branch above
 * lam = 12), word 1 that branch's angle, words 2, 3 the read-noise normal.  frame = the number of observations the handle has written so
 * far: every aog_reset* / aog_step* call adds one, with or without a detector; a masked aog_reset counts as one frame, draws for the masked
 * envs only and leaves the other rows of obs_raw / obs untouched.  The count travels in the state blob.  Nothing else enters (route, launch
 * shape, fused or separate launches, batch split).
 * photons_host = NULL switches the detector off: the handle then launches the kernels it launched before, with the same arguments.
 * AOG_ERR_UNSUPPORTED (naming the sizes) when the table route's epilogue cannot hold the noisy plane in LDS beside the clean powers. */
int aog_set_detector(aog_env* env, const double* photons_host, const double* read_noise_host, const double* background_host, void* stream);
/* The per-env values aog_set_turbulence derives, for `count` Cn^2 values (pure host function, no handle or device): two-band sample
 * amplitudes (high / low band), literal-route crop scale, sqrt(Cn^2), int8 noise scale sqrt(Cn^2) / table_sqrt_cn_squared.  Null outputs
 * are skipped. */
int aog_turbulence_factors(int n_pupil, int oversampling, double pixel_pitch, const double* cn_squared, int count, double table_sqrt_cn_squared,
                           float* amp_high, float* amp_low, float* crop_scale, double* sqrt_cn_squared, double* x8_noise_scale);

/* The launch form aog_create chooses for the fused pupil pass of a fast matrix-core handle (pure host function, no handle or device; ABI
 * stays 22, no new struct): the values the constructor and the launcher compute, from the same definition.  four_wave: as the environment
 * variable AOG_FUSED_4WAVE.  out[AOG_FUSED_PLAN_FIELDS], in this order: env tiles per workgroup, waves per workgroup, heavy share (x / 1024,
 * 0 = interleaved sub-chunks), workgroups per pixel chunk, paired workgroup map (0 / 1), pixel chunks, longest chunk in pixel tiles, partial
 * slabs (aog_info.pixel_chunks), pixel tiles, env tiles, padded mode count, padded table count, bytes of dynamic LDS per workgroup when the
 * screens come from the packed tiles (every static handle; a dynamic one that repacks), the same when a dynamic handle reads its ring
 * directly (equal to the former for atm_dynamic = 0: aog_create does not know yet which of the two a dynamic handle gets), and the vector
 * kernel's pixel quads per chunk and chunks.  AOG_ERR_UNSUPPORTED, with the message aog_create gives, for a shape no form fits. */
#define AOG_FUSED_PLAN_FIELDS 16
int aog_fused_plan(int num_envs, int n_ap, int n_modes, int n_wfs_tables, int atm_dynamic, int pixel_chunks, int four_wave, int32_t* out);

/* The split-f16 operand tiles of the matrix Fourier transform family (K4, K11, K13, K14, K15), as the library's one host packer lays them out
 * (pure host functions, no handle or device; ABI stays 22, no new struct; tests/test_operand_tiles_cpu.py holds them to the numpy packers of
 * pyramid_host.py).  One tile = [re hi, re lo, im hi, im lo][lane 64][8] IEEE halves; a table holds a matrix m [i][k] as [n_blocks][k_pad / 16]
 * tiles, tile (i >> 5, k >> 4), with k in one of two orders:
 *   AOG_TILE_NATURAL      lane (i & 31) + 32 ((k >> 3) & 1), slot k & 7
 *   AOG_TILE_ACCUMULATOR  lane (i & 31) + 32 ((k >> 2) & 1), slot (k & 3) + 4 ((k >> 3) & 1)   (the order a matrix-core accumulator holds rows)
 * aog_pack_operand_tiles: tiles_out [n_blocks][k_pad / 16][4][64][8] <- m [rows][K] complex float64 (re, im interleaved) x scale; hi = the value
 * rounded to half through float, lo = the float64 remainder rounded the same way; the pads (i >= rows, k >= K) are zero.
 * aog_reorder_operand_tiles: dst <- the tiles of the TRANSPOSED matrix of the packed table src, in another order and shape: element (i, k) of
 * dst is element (k, i) of src, halves copied as they are (what aog_pyramid_gradient does to the uploaded tables), zero where src has none.
 * AOG_ERR_INVALID for an unknown order, k_pad no positive multiple of 16, or a matrix that does not fit. */
enum { AOG_TILE_NATURAL = 0, AOG_TILE_ACCUMULATOR = 1 };
int aog_pack_operand_tiles(const double* m, int rows, int K, double scale, int order, int n_blocks, int k_pad, uint16_t* tiles_out);
int aog_reorder_operand_tiles(const uint16_t* src, int src_order, int src_blocks, int src_k_pad, int dst_order, int dst_blocks, int dst_k_pad,
                              uint16_t* dst);

/* How aog_generate_screens draws a screen.  Both methods draw the same zero-mean stationary Gaussian field on the N x N pupil up to
 * max |dC(r)| < 1e-4 C(0) over every lag r of the pupil (tests/test_screen_twoband.py evaluates both covariance functions exactly on
 * the host in float64), i.e. they are statistically equivalent to hcipy's layer.reset() (AO_env.py:77), not draw-for-draw.
 *   AOG_SCREENS_TWOBAND (default)  the spectrum samples' variance is split by a smooth radial window into a low band kept on hcipy's
 *       (oversampling N)^2 frequency grid (non-zero below 2 cycles per pupil diameter: 4 oversampling^2 samples) and a high band drawn
 *       on the (2 N)^2 grid (period 2 D: its covariance has decayed before the wrap-around lag).  4 N^2 + 4 q^2 samples per screen
 *       instead of q^2 N^2.  Needs oversampling >= 4 and even, N % 4 == 0; otherwise the literal method is used.
 *   AOG_SCREENS_HCIPY  the literal (oversampling N)^2 draw described above. */
enum { AOG_SCREENS_TWOBAND = 0, AOG_SCREENS_HCIPY = 1 };
int aog_set_screen_method(aog_env* env, int method);

/* Shack-Hartmann baseline controller (AO_env.py:254-290, 396-465).  Tables built on the host by the counterpart of
 * shack_hartmann_init (adaptive_optics_gym_amd/sh_host.py).  HOST pointers, float64. */
typedef struct {
  int32_t n_sub;                /* flux-selected sub-apertures (AO_env.py:418-425)                                 */
  const int32_t* sub_slot;      /* [N*N] slot 0..n_sub-1 of the pixel's lenslet, or -1                             */
  const double* centres;        /* [n_sub][2] lenslet positions (x, y) the estimator subtracts                      */
  const double* slopes_ref;     /* [2 n_sub] reference slopes, all x then all y (AO_env.py:428)                     */
  const double* reconstruction; /* [A][2 n_sub] inverse_tikhonov(response, 1e-3) (AO_env.py:464-465)                */
  const double* mla_phase;      /* [N*N][2] exp(i k opd) of the micro-lens array                                    */
  const double* transfer;       /* [2N][2N][2] Fresnel transfer function on the unshifted 2x-padded FFT grid        */
  const double* x_det;          /* [N] detector coordinate of a column / row (NoiselessDetector(focal_grid))        */
  double field_amplitude;       /* amplitude of wf_wfs on the aperture / magnification                              */
  double image_scale;           /* magnified pixel area x delta_t: image = |E|^2 * image_scale                      */
  double gain, leakage;         /* 0.3, 0.01 (AO_env.py:282-283)                                                    */
  int32_t fft_double;           /* 0 (default): the Fresnel propagation runs complex64 transforms — relative error ~1e-6 of the image
                                   peak, far below the photon noise (>= 1e-3) large_poisson adds before anything reads the image;
                                   1: complex128 transforms (bit-for-bit comparisons of the noise-free image with a float64 oracle) */
  int32_t reserved0;
} aog_sh_tables;
int aog_upload_sh(aog_env* env, const aog_sh_tables* sh);

/* camera.integrate(shwfs(magnifier(deformable_mirror_shack(layer(wf_wfs)))), delta_t); camera.read_out() (AO_env.py:263-274):
 * the noise-free Shack-Hartmann image of every env, [B][N*N] float64.  image_dev may be NULL = "the next call is aog_sh_update(NULL)":
 * the image stays internal, and for pupils of 128 / 240 / 256 / 480 / 512 pixels (complex64) it is not even written — photon noise and the
 * estimator's per-lenslet sums are taken inside the last propagation pass and handed to that aog_sh_update. */
int aog_sh_image(aog_env* env, double* image_dev, void* stream);

/* large_poisson + estimate + slopes_ref + leaky integrator (AO_env.py:275-287) -> deformable_mirror_shack.actuators, which
 * are also returned in action_dev [B][A] float64 (the action SH_step hands to step()).  noisy_image_dev: the image after the
 * caller's own large_poisson (parity with a host RNG stream), or NULL = photon noise from the handle's Philox stream. */
int aog_sh_update(aog_env* env, const double* noisy_image_dev, double* action_dev, void* stream);

/* Checkpointing (the reference has none for the env): every piece of per-env state the handle owns — screens
 * (and ring-buffer origins / RNG stream positions for dynamic handles), mirror and Shack-Hartmann actuators, per-episode step
 * counters — as one opaque device blob of aog_state_bytes() bytes, plus the global step counter.  A blob is only valid for a
 * handle created with the same configuration.  Its last 256 bytes carry the host-side positions of the device random streams: the seed,
 * the Shack-Hartmann call count, the steps since the reset, the detector's frame and the pyramid sensor's frame.  Not in it, and left as
 * they are by aog_set_state: the science camera's exposure and frame counts (measurement data), the return accumulator's tensor (the
 * caller's) and the profiling records. */
int64_t aog_state_bytes(const aog_env* env);
int aog_get_state(aog_env* env, void* blob_dev, int64_t* timestep_out, void* stream);
int aog_set_state(aog_env* env, const void* blob_dev, int64_t timestep, void* stream);

/* The sensing-arm pupil phase of one env in radians on the full N x N grid (0 outside the aperture, aperture mean removed):
 * atmosphere only (what render() shows as the phase screen, AO_env.py:87-88,128-129).  float32 [N*N]. */
int aog_get_phase_screen(aog_env* env, int env_index, float* phase_dev, void* stream);

/* Episode-return accumulation of the rollout (algorithm.py:509-510 sums the rewards of an episode on the host): when
 * returns_dev ([B] float32, caller-owned, device) is set, every aog_step also does returns_dev[env] += reward[env] (float32, the
 * same arithmetic as the caller's own `returns += reward`) in its last kernel.  NULL detaches.  The caller zeroes the buffer at
 * episode start and reads it (all-gathers it across ranks) at episode end. */
int aog_set_return_accumulator(aog_env* env, float* returns_dev);

/* Synchronises the device and returns the handle's sticky device-side status word: 0 = fine, 1 = a bounded inter-workgroup wait
 * timed out (results of that step are invalid).  The library also watches the same flag through pinned host memory without
 * synchronising: once it is set, aog_step and aog_reset fail with AOG_ERR_STATE (at the latest from the call after the one whose
 * launch tripped it) until new screens are installed for the whole batch (aog_set_screens_*) or a state is restored. */
int aog_device_status(aog_env* env, int32_t* status_out);

/* deformable_mirror.actuators for all envs (metres; AO_env.py:116).  [B][A] float64 device pointers. */
int aog_get_actuators(aog_env* env, double* act_dev, void* stream);
int aog_set_actuators(aog_env* env, const double* act_dev, void* stream);

/* AOEnv.reset (AO_env.py:74-103) for the envs with mask_dev[b] != 0 (NULL = all): flatten the mirror iff
 * flat_mirror_start, zero the per-episode step counter, and return the observation of EVERY env
 * (obs_raw_dev [B][o^2] float32 before the cast, obs_dev [B][o^2] IEEE half; either may be NULL).
 * A masked reset is only bound to write the rows of the envs it selects: hand in buffers whose other rows hold those envs' last observation
 * (which is what the call would write there).  Handles whose reset observation cannot change between episodes (static screens, flat start,
 * table route, no detector) keep it after the first unmasked reset and answer later resets, masked or not, from that copy in one launch,
 * until screens, tables, turbulence values or a state are installed; AOG_RESET_CACHE=0 at aog_create switches this off (same results). */
int aog_reset(aog_env* env, const uint8_t* mask_dev, float* obs_raw_dev, uint16_t* obs_dev, void* stream);

/* AOEnv.step (AO_env.py:106-153) incl. reward_function (AO_env.py:468-503).
 *   action_dev  [B][A] float32
 *   obs_raw_dev [B][o^2] float32 (wf.power before the float16 cast, AO_env.py:142)   nullable
 *   obs_dev     [B][o^2] IEEE half (AO_env.py:153)                                   nullable
 *   reward_dev  [B] float32;  done_dev [B] uint8;  power_dev [B] float32 (info["power"])
 *   strehl_dev  [B] float32 (Strehl ratio in [0,1]; nullable) */
int aog_step(aog_env* env, const float* action_dev, float* obs_raw_dev, uint16_t* obs_dev, float* reward_dev,
             uint8_t* done_dev, float* power_dev, float* strehl_dev, void* stream);

/* aog_step for callers that know the NEXT action when they hand over the current one (open-loop action sequences, replayed trajectories,
 * throughput benchmarks on synthetic actions): identical results, one kernel launch less per step.  The last launch of the call carries
 * the epilogue of this step AND the action -> actuator prologue of the next one (they share nothing); the next call then skips its own
 * prologue and `action` must be the `action_next` of the call before (it is not looked at).  action_next = NULL ends the sequence (a plain
 * epilogue).  Between a call with action_next != NULL and the next call the mirror state already belongs to the next step: aog_reset,
 * aog_step, aog_get_state, aog_get_actuators, aog_focal_image(s), aog_sh_* ... fail with AOG_ERR_STATE until the sequence is ended
 * (aog_set_actuators / aog_set_state replace the mirror and end it).  Not together with aog_set_lookahead.  (ABI 17) */
int aog_step_pipelined(aog_env* env, const float* action_dev, const float* action_next_dev, float* obs_raw_dev, uint16_t* obs_dev, float* reward_dev,
                       uint8_t* done_dev, float* power_dev, float* strehl_dev, void* stream);

/* self.wf_wfs_after_foc.electric_field of one env (AO_env.py:138): the n_focal x n_focal focal-plane field of the sensing
 * arm with the current screen and mirror, as interleaved (re, im) float32, row-major (y, x), up to a global phase (the
 * library stores screens with their aperture mean removed).  Off the step() path; used for render()/fiber cross-checks. */
int aog_focal_image(aog_env* env, int env_index, float* field_dev /* [n_focal][n_focal][2] */, void* stream);

/* The same field for envs [first, first + count) in one call: field_dev [count][n_focal][n_focal][2] float32.  Fast-precision handles
 * only.  E = exp(i phi) on the pupil grid from the split-f16 phase contraction of the step kernels, then the two matrices of the
 * Fraunhofer matrix Fourier transform as two batched complex products on the f16 matrix cores (v_mfma_f32_32x32x16_f16, every operand split
 * hi + lo: 22 significant bits per factor, exact products), the pupil field formed inside the first product from a dense phase grid. */
int aog_focal_images(aog_env* env, int first, int count, float* field_dev, void* stream);

/* ---- residual wavefront statistics and the best-fit mirror command (no counterpart in the reference: the truth a controller is read against) ----
 * Per env, over the n packed aperture pixels p, in float64: w_p = s_p / (2 pi) + 2 (M a)_p is the optical path error in metres (s = the
 * achromatic screen, M = aog_tables.modes, a = the current actuators), rms = std_p(w), Mc = M - its column means over the aperture,
 * b = Mc' w, c = P b with P = pinv(Mc' Mc) the least-squares coefficients of w on the modes (metres of path),
 * fit_rms = sqrt(max(0, rms^2 - b' c / n)) the RMS the best correction leaves, act_ideal = a - c / 2 (path = 2 x surface).
 *
 * Host tables of the wavefront fit, float64 HOST pointers: the mode matrix again
 * (the library keeps no host copy) and P [A][A].  After aog_upload_tables; a later
 * aog_upload_tables clears them.  Builds the modes' table-operand layout (split f16,
 * tab16's order, A_pad rows) and the column sums; the buffers are allocated here, not
 * at aog_create, so handles that never ask keep their device_bytes. */
int aog_upload_wavefront_fit(aog_env* env, const double* modes_host, const double* fit_host);

/* rms, fit_rms [B]; coef, act_ideal [B][A]; float64 device pointers, each nullable
 * (at least one non-NULL).  Whole batch, stream-ordered, no host synchronisation.
 * Fast handles: the split-f16 phase contraction of the step kernels fused with a second matrix-core contraction of that phase against the
 * modes, float64 sums in a fixed order (a batch split over handles reproduces the whole batch bit for bit); float64 validation handles: a
 * plain float64 kernel.  Reads the state the last reset or step left and changes nothing a step reads or writes (its partial sums live in
 * a buffer of its own, its actuator operands in the scratch the off-step instruments of a handle share; the first call allocates both).  AOG_ERR_STATE before tables, screens or the fit are installed,
 * while a pipelined or policy-attached step has an action pending, and between two steps of a lookahead episode. */
int aog_wavefront_truth(aog_env* env, double* rms_dev, double* fit_rms_dev,
                        double* coef_dev, double* act_ideal_dev, void* stream);

/* ---- science camera: long-exposure PSF, Strehl and encircled energy (the image AO_env.py:479 forms every step and reads one pixel of) ----
 * The camera sees a centred window of w x w samples of the science arm's focal grid (make_focal_grid(q, num_airy, lambda_sci / D): n_s =
 * 2 q num_airy samples per axis, on-axis sample c = n_s / 2): rows and columns [c - w/2, c + w/2), w even.  A frame of an env is
 *   I[v][u] = | sum_{y,x} m1[v][y] E[y][x] m2[x][u] |^2,  E = exp(2 pi i u_p phase_ratio) on the aperture, 0 outside,
 * u_p the residual phase in revolutions of the sensing wavelength (screen + mirror, as the step kernels form it), phase_ratio =
 * lambda_wfs / lambda_sci.  m1, m2 are the window's Fraunhofer matrices with the normalisation folded into m1 so that a flat wavefront
 * gives I[w/2][w/2] = 1: a frame's centre pixel IS that step's Strehl ratio, and I = wf_sci_focal_plane.power / (unaberrated_PSF.max() x
 * total power).  Per env the library keeps the float64 sum of the integrated frames (the exposure) and their number.  Neither is part of
 * the aog_get_state blob: a restored state continues with whatever the camera holds.
 *
 * Host tables, float64 / int32 HOST pointers: m1 [w][N][2], m2 [N][w][2] (re, im), ee_bin [w*w] the radial bin 0 .. n_ee - 1 of each
 * window pixel (-1 = outside every radius), peak_fraction = the unaberrated peak's share of the beam's power (unaberrated_PSF.max() of a
 * unit-power beam).  After aog_upload_tables; a later aog_upload_tables clears the camera.  Builds the split-f16 operand tables of the
 * matrix-core path; every buffer of the camera is allocated here, not at aog_create, so handles that never ask keep their device_bytes
 * (the actuator operands of a call are the scratch the off-step instruments of a handle share, made by the first call that needs it).
 * A second upload replaces the first (and its exposures).  AOG_ERR_INVALID for an odd window, one outside [2, 4096] or n_ee outside
 * [1, 32].  The focal grid's size n_s is not part of aog_config — m1 / m2 define the grid — so w <= n_s is the caller's to hold
 * (BatchedAOEnv raises ValueError above 240); the library's cap bounds the exposure's size only.  phase_ratio is used as given on fast
 * and float64 handles alike. */
int aog_upload_science(aog_env* env, const double* m1_host, const double* m2_host, int window, double phase_ratio, double peak_fraction,
                       const int32_t* ee_bin_host, int n_ee);

/* Add the current frame of every env (mask_dev: nullable [B] uint8 device array, non-zero = selected) to its exposure and count it.
 * Stream-ordered, no host synchronisation; frames add in stream order, one thread owns one pixel (no atomics), so an exposure does not
 * depend on how the envs are grouped into handles, masks or chunks.  Fast handles: a phase grid at the science wavelength (the
 * split-f16 phase contraction of the step kernels, scaled by phase_ratio before it is reduced to a revolution), then K4's two
 * matrix-core products on the window's geometry, the second squaring its accumulators into the exposure instead of writing a field.
 * Float64 validation handles: per env, plain float64 kernels.  Reads the state the last reset or step left and changes nothing a step
 * reads or writes (actuator operands and work buffers are the camera's own).  AOG_ERR_STATE before tables, screens or aog_upload_science,
 * while a pipelined or policy-attached step has an action pending, and between two steps of a lookahead episode. */
int aog_science_integrate(aog_env* env, const uint8_t* mask_dev, void* stream);

/* Zero the exposure and frame count of the selected envs (mask_dev as above).  Same preconditions. */
int aog_science_clear(aog_env* env, const uint8_t* mask_dev, void* stream);

/* Read envs [first, first + count): psf [count][w][w] the mean frame (exposure / frames), strehl [count] its centre pixel, ee
 * [count][n_ee] the encircled energy EE_k = peak_fraction x sum of the mean frame over the pixels of bins <= k (a share of the beam's
 * power), frames [count] int32.  float64 device pointers but frames_dev; each nullable, at least one non-NULL.  Sums run in float64 in a
 * fixed order per env.  An env with no frames reads as zeros.  Stream-ordered; same preconditions. */
int aog_science_read(aog_env* env, int first, int count, double* psf_dev, double* strehl_dev, double* ee_dev, int32_t* frames_dev,
                     void* stream);

/* ---- analytic gradient of observation, power and Strehl with respect to the mirror (no counterpart in the reference) ----
 * The atmosphere never depends on the action and AOEnv.step sets the mirror absolutely (AO_env.py:115-120): every output of step t depends
 * on the policy through action t alone, so this one-step vector-Jacobian product is the whole differentiable simulator.
 * With the names of aog_tables — phi_p the sensing-arm phase in radians on packed aperture pixel p, E_p = exp(i phi_p),
 * Z_j = sum_m coef[j][m] sum_p E_p g_m(p) — and the cotangents gbar_j (g_obs for the rows of the observation, g_power for every fiber-mode
 * row), the call differentiates  L = sum_j gbar_j |Z_j|^2 + g_strehl |Z_sci|^2  per env:
 *     C_m     = sum_j gbar_j conj(Z_j) coef[j][m]
 *     H_p     = sum_m C_m g_m(p)
 *     q_p     = 2 Re(i E_p H_p)                         = dL/dphi_p
 *     dL/da_k = (4 pi / lambda_wfs) sum_p M_pk q_p      (a = actuators, metres of surface; M = aog_tables.modes)
 * The science arm is the same with sci_tables, sci_coef and E^sci_p = exp(i r phi_p), r = lambda_wfs / lambda_sci; its q_p carries an extra
 * factor r.  Action chain (AO_env.py:119-120): v_k = action_k / (k + 10), n = sqrt(v' G v) with G = aog_tables.gram, c =
 * cfg.surface_rms_target, a = c v / n; with g = dL/da:  dL/dv = (c / n) (g - (g . v) (G v) / n^2),  dL/daction_k = (dL/dv)_k / (k + 10), in
 * float64 without fused multiply-add.  A zero action gives NaN, as the forward does.  The outputs are invariant to the action's scale, so
 * action . dL/daction = 0.  The detector (aog_set_detector) does not enter: the gradient is of the clean outputs.
 *
 * Host tables of the gradient: the aog_tables given to aog_upload_tables, again (the library keeps no host copy; modes, wfs_tables and
 * sci_tables are read).  After aog_upload_tables; a later aog_upload_tables clears the upload.  Fast handles build the operand tables of
 * the matrix-core kernels here (the wfs tables as forward operands and transposed, the modes as table operands); every buffer is allocated
 * here or by the first aog_output_gradient, so handles that never ask keep their device_bytes. */
int aog_upload_gradient(aog_env* env, const aog_tables* tables);

/* The vector-Jacobian product at the state the last reset / step left.
 * cotangents (float64 device, each nullable, at least one non-NULL): g_obs [B][o^2], g_power [B], g_strehl [B]
 * outputs (float64 device, each nullable, at least one non-NULL):
 *   grad_act [B][A]      dL/d actuators (per metre of surface)
 *   grad_action [B][A]   dL/d action through the chain above (needs action_dev [B][A] float32, the action that produced the current
 *                        actuators; AOG_ERR_INVALID on sh_operation handles or without action_dev)
 *   values [B][o^2 + 2]  the float64 obs_raw, power, Strehl the gradient was taken at (the forward of this call; on the separable
 *                        observation route the o^2 observation entries are NaN)
 * Whole batch, stream-ordered, no host synchronisation, no atomics; an env's results depend on its own operands only, so a batch split
 * over two handles reproduces the whole batch bit for bit.  Fast handles: a forward pupil pass of the call's own (the step's partial sums
 * are not read), a float64 kernel per env for Z, the values and C, the pupil pass backwards on the matrix cores, a finish kernel; float64
 * validation handles: plain float64 kernels.  Reads the state the last reset or step left and changes nothing a step reads or writes.
 * AOG_ERR_STATE before tables, screens or aog_upload_gradient, while a pipelined or policy-attached step has an action pending, between
 * two steps of a lookahead episode and on a poisoned handle.  On separable-observation handles (cfg.obs_separable = 1) g_obs must be NULL
 * (AOG_ERR_UNSUPPORTED otherwise) unless aog_upload_gradient_obs was called; power and Strehl gradients work there either way, because the
 * wfs tables are the fiber modes. */
int aog_output_gradient(aog_env* env, const double* g_obs_dev, const double* g_power_dev, const double* g_strehl_dev,
                        const float* action_dev, double* grad_act_dev, double* grad_action_dev, double* values_dev, void* stream);

/* The observation gradient on the separable route (obs_dim 6 .. 32 of fast handles, >= 8 of float64 handles; additive in ABI 22).  There the
 * observation is no row of wfs_coef but the matrix Fourier transform of aog_obs_mft, and its part of the gradient is, per env on the pupil grid,
 *     E = A o exp(i phi)            phi the sensing-arm phase above, A the aperture
 *     F = m1 E m2                   o x o; obs_raw[v * o + u] = |F_vu|^2, row v * o + u as in aog_obs_mft
 *     W = gbar o conj(F)            gbar = g_obs
 *     H = m1' W m2'                 N x N, ' the plain transpose
 *     q_yx = 2 Re(i E_yx H_yx)      on aperture pixels
 * and this q adds to the q_p of power and Strehl before dL/da_k = (4 pi / lambda_wfs) sum_p M_pk q_p; the action chain is unchanged and the
 * detector does not enter.  Opt-in per handle: after aog_upload_tables, aog_upload_obs_mft and aog_upload_gradient, on handles with
 * cfg.obs_separable = 1 only (AOG_ERR_STATE otherwise), with the same HOST matrices as aog_upload_obs_mft (the library keeps no host copy); a
 * later aog_upload_tables clears it.  With it aog_output_gradient accepts g_obs [B][o^2] and writes the float64 obs_raw into values[:, :o^2]
 * (the forward of the call: K11's pass 1, then float64 sums over the k-steps of pass 2).  With g_obs == NULL grad_act / grad_action and
 * values[:, o^2:] are bit for bit those of a handle without the upload; a handle without it keeps the refusal, the NaN and its launches.
 * Fast handles: W is scaled by a power of two per env and split into f16 operands, H = m1' (W m2') runs on the matrix cores one wave per
 * (env, 32 x 32 tile of the grid) and leaves q in place of the phase, a second kernel gathers q per (env tile, pixel tile) and contracts it
 * with the modes into partial sums that the finish kernel adds in a fixed order: no atomics, an env's result depends on its own operands
 * only, and neither a split of the batch over handles nor the round size changes a bit.  The phase grid and T' go through the step's own
 * observation work buffers (every step rewrites them in full before it reads them); the other buffers are allocated here or by the first
 * call and counted in device_bytes.  Rounds of whole env tiles: as many envs as those work buffers hold, or fewer with the environment
 * variable AOG_GRAD_OBS_CHUNK (read here).  Float64 handles: one env at a time, plain float64 products. */
int aog_upload_gradient_obs(aog_env* env, const aog_obs_mft* mft);

/* ---- modulated pyramid wavefront sensor (additive in ABI 22; no counterpart in the reference) ----
 * Per env, E = exp(2 pi i u) on the aperture (u = screen + mirror phase in revolutions of lambda_wfs, as the step kernels form it).  For
 * each of n_mod modulation points j the focal field on a w x w window (w = 2 samples) is the matrix Fourier transform F_j = m1_j E m2_j,
 * the modulation tilt folded into the matrices; quadrant (s_y, s_x) of F_j is carried back to an n_s x n_s pupil image G = b1_{s_y} F_j
 * b2_{s_x} (b1 / b2 hold zeros outside their half of the window, so every product runs over the whole window), and the frame is
 *   I[q][y][x] = (1 / n_mod) sum_j |G_{q,j}[y][x]|^2,   q = 2 (s_y > 0) + (s_x > 0),   float64, j ascending.
 * With photons > 0 every pixel is replaced by large_poisson(photons x I) / photons from ONE Philox4x32-10 call keyed by the handle's rng_seed
 * with counter {q n_s^2 + y n_s + x, global env id, frame & 0xFFFFFFFF, (frame >> 32) ^ 0x9F2A31D}, frame = the number of sensor calls
 * (aog_pyramid_frames / _slopes / _update) made on the handle since the upload: word 0 is the Poisson uniform or the Box-Muller radius, word
 * 1 the angle.  Slopes over the n_valid pixels of `valid` (indices y n_s + x, ascending):
 *   s_x[k] = (I[1] + I[3] - I[0] - I[2])[valid k] / Ibar,  s_y[k] = (I[2] + I[3] - I[0] - I[1])[valid k] / Ibar,
 *   Ibar = mean over the valid pixels of I[0] + I[1] + I[2] + I[3];   slopes [B][2 n_valid] = s_x then s_y.
 * All host tables are HOST pointers.  float64: m1 [n_mod][w][N][2], m2 [n_mod][N][w][2], b1 [2][n_s][w][2], b2 [2][w][n_s][2] (index 0: the
 * k < 0 half).  Split-f16 operand tiles for fast handles (IEEE half bits; one tile = [re hi, re lo, im hi, im lo][lane 64][8]): m1s per j
 * in the science camera's m1s layout [ceil(w/32)][ceil(N/16)] tiles, m2s per j in its m2s layout [ceil(w/32)][Nxp/32][2] tiles (Nxp = N
 * rounded up to 128), b1s [2][ceil(n_s/32)][ceil(w/32)][2] and b2s likewise in the m2s layout with the window index in the place of x (the
 * order accumulator registers hold it); fwd_unscale / back_unscale: what undoes the powers of two the forward / back tables were scaled
 * by (both products of a pair).  Float64 validation handles read the float64 tables, fast handles the operand tiles.  The struct is
 * four int32, nine pointers and three doubles in natural alignment; it has no index in aog_struct_size. */
typedef struct aog_pyramid_tables {
  int32_t samples;      /* w_q: focal samples per quadrant side, 8 .. 64 */
  int32_t pixels;       /* n_s: detector pixels per image side, 8 .. 64 and <= n_pupil */
  int32_t n_mod;        /* 1 .. 32 */
  int32_t n_valid;      /* 1 .. n_s^2 */
  const double* m1;
  const double* m2;
  const double* b1;
  const double* b2;
  const uint16_t* m1s;
  const uint16_t* m2s;
  const uint16_t* b1s;
  const uint16_t* b2s;
  const int32_t* valid; /* [n_valid] */
  double fwd_unscale;
  double back_unscale;
  double photons;       /* expected photo-electrons per frame of a beam that puts 1 into every pixel (0: no photon noise) */
} aog_pyramid_tables;

/* Install the sensor.  After aog_upload_tables (a later aog_upload_tables clears it); every buffer of the sensor is allocated here (but
 * the actuator operands of a call: the off-step instruments' shared scratch, made by the first call that needs it), so handles that never
 * ask keep their device_bytes and their launches.  A second upload replaces the first and restarts the frame count; aog_set_state
 * restores the count its blob was saved with, so upload the sensor before a state is restored, not after.
 * Work proceeds in chunks of whole env tiles, capped at ~256 MB per work buffer or at the environment variable AOG_PYRAMID_CHUNK (read
 * here).  AOG_ERR_INVALID for a size outside the ranges above, a bad valid index or a non-finite / negative photons. */
int aog_upload_pyramid(aog_env* env, const aog_pyramid_tables* tables);

/* The frame of every env (mask_dev: nullable [B] uint8 device array, non-zero = selected; the rows of the others are not touched) into
 * frames_dev [B][4][n_s][n_s] float64.  Stream-ordered, no host synchronisation, no atomics: an env's frame depends on its own operands
 * only, not on how envs are grouped into handles, masks or chunks.  Fast handles: the phase grid once, then per modulation point the
 * science camera's two matrix-core passes (the second storing the field as split-f16 operands) and one wave per (env, quadrant) for both
 * back products; float64 handles: plain float64 kernels per env.  Reads the state the last reset or step left and changes nothing a step
 * reads or writes.  AOG_ERR_STATE before tables, screens or aog_upload_pyramid, while a pipelined or policy-attached step has an action
 * pending, and between two steps of a lookahead episode. */
int aog_pyramid_frames(aog_env* env, const uint8_t* mask_dev, double* frames_dev, void* stream);

/* The same call, finished to slopes_dev [B][2 n_valid] float64 (frames stay in a buffer of the sensor). */
int aog_pyramid_slopes(aog_env* env, const uint8_t* mask_dev, double* slopes_dev, void* stream);

/* Reconstructor R [A][2 n_valid] and reference slopes s_ref [2 n_valid], float64 HOST pointers.  After aog_upload_pyramid. */
int aog_upload_pyramid_reconstructor(aog_env* env, const double* recon_host, const double* slopes_ref_host);

/* One sensor call, then the integrator act_out[e][k] = a[e][k] - gain sum_i R[k][i] (s[e][i] - s_ref[i]) with a the current actuators, into
 * act_out_dev [B][A] float64 (float64 sums over i ascending, no fused multiply-add).  The mirror itself is not touched: the caller steps
 * with act_out.  slopes_dev: nullable [B][2 n_valid], the slopes it used.  AOG_ERR_STATE before aog_upload_pyramid_reconstructor. */
int aog_pyramid_update(aog_env* env, double gain, double* act_out_dev, double* slopes_dev, void* stream);

/* The vector-Jacobian product of the sensor's CLEAN frame and slopes with respect to the mirror's actuators (per metre of surface, the
 * units of aog_get_actuators): grad_dev [B][A] float64 = d/da of sum(g_frames * frame) + sum(g_slopes * slopes).  g_frames_dev: nullable
 * [B][4][n_s][n_s]; g_slopes_dev: nullable [B][2 n_valid]; at least one (AOG_ERR_INVALID), both add.  A slopes cotangent is pulled back to
 * the frame in float64 through s_x = (I1 + I3 - I0 - I2) / Ibar, s_y = (I2 + I3 - I0 - I1) / Ibar, the dependence on Ibar included.
 * act_dev: nullable [B][A], the point of evaluation instead of the mirror's actuators (the mirror is never written).  frames_dev /
 * slopes_dev: nullable, the clean frame and slopes at that point, from the launches of aog_pyramid_frames (the same bits as that call
 * gives without photons).  With W_{q,j} = g_q o conj(G_{q,j}) / n_mod, V_j the window whose quadrant block q is b1' W_{q,j} b2', and
 * H_j = m1_j' V_j m2_j' (' = the plain transpose): q_p = sum_j 2 Re(2 pi i E_p H_{j,p}) on the aperture, j ascending, and
 * grad_k = (2 / lambda_wfs) sum_p M_pk q_p.  Photon noise is not differentiated: the call draws no random number and leaves the sensor's
 * frame count alone.  mask_dev as above: the rows of the envs it leaves out are not touched, in any output.  Stream-ordered, no host
 * synchronisation, no atomics; an env's result depends on its own operands only.  The work buffers are allocated by the first call (which
 * blocks for that): a handle that never asks keeps its device_bytes.  grad_dev may be NULL when both cotangents are NULL and frames_dev or
 * slopes_dev is given: the clean values alone.  Fast handles: per chunk the phase grid once, per modulation point the two forward passes,
 * k_pyr_grad_back (one wave per (env, quadrant): G again, W, back through b1' and b2' on the matrix cores) and k_pyr_grad_q (back through
 * m2_j' and m1_j', added into an fp32 q grid; every split operand first brought into a fixed binade by a measured power of two), then
 * the modes contraction of aog_output_gradient's separable route; they need
 * aog_upload_gradient (AOG_ERR_STATE without) and are built for w_q <= 32, n_s <= 64 (AOG_ERR_UNSUPPORTED beyond, the sizes named).
 * Float64 handles: plain float64 kernels per env.  Refusals as aog_pyramid_frames. */
int aog_pyramid_gradient(aog_env* env, const uint8_t* mask_dev, const double* g_frames_dev, const double* g_slopes_dev, const double* act_dev,
                         double* grad_dev, double* frames_dev, double* slopes_dev, void* stream);

/* ---- policy query of the rollout (Actor.forward + Actor.get_action, network.py:17-69; caller algorithm.py:216-296) ----
 * mean = W_o drop(relu(W_3 drop(relu(W_2 drop(relu(W_1 obs + b_1)) + b_2)) + b_3)) + b_o with nn.Dropout(dropout_p) ACTIVE
 * (the reference never leaves training mode while acting), action = mean + sqrt(cov_var) eps, eps ~ N(0, I),
 * log_prob = MultivariateNormal(mean, cov_var I).log_prob(action).  Weights are torch nn.Linear layouts [out][in], float32,
 * device pointers; they are read on every call (the learner updates them between rollouts).  Dropout masks and eps come from
 * Philox4x32-10 keyed by (seed, call_index, global env id, layer, unit): statistically, not bit-wise, torch's streams.
 * One launch per call; independent of any aog_env handle. */
typedef struct aog_actor {
  int32_t batch, state_dim, hidden_dim, act_dim;
  int32_t env_id_base;                  /* global id of obs row 0: dropout masks and eps are keyed by the GLOBAL env id */
  int32_t reserved0;                    /* = 0 */
  const float* w1; const float* b1;     /* [hidden][state],  [hidden] */
  const float* w2; const float* b2;     /* [hidden][hidden], [hidden] */
  const float* w3; const float* b3;     /* [hidden][hidden], [hidden] */
  const float* wo; const float* bo;     /* [act][hidden],    [act]    */
  float dropout_p;                      /* 0.5 in the reference (network.py:39); 0 = evaluation mode */
  float cov_var;                        /* 0.5 in the reference (algorithm.py:107) */
  uint64_t seed, call_index;
} aog_actor;
/* obs: [batch][state_dim], float16 bits (obs_is_f16 = 1: what aog_step writes) or float32; outputs may be NULL. */
int aog_actor_act(const aog_actor* net, int device, const void* obs_dev, int obs_is_f16, float* mean_dev /* [batch][act] */,
                  float* action_dev /* [batch][act] */, float* log_prob_dev /* [batch] */, void* stream);

/* ---- action forms of the policy query: evaluation (the mean) and DDPG's exploration noise (algorithm.py:258-259, network.py:259-274) ----
 * For each (env < batch, unit) let g = the float32 action of aog_actor_act (mean + sqrt(cov_var) eps).
 *   mode  AOG_ACTION_SAMPLE: g as is.  AOG_ACTION_MEAN: g = mean (the same float as mean_dev), dropout as net->dropout_p says, no eps;
 *         log_prob = the density of N(mean, cov_var I) at the mean = -0.5 act_dim log(2 pi cov_var).
 *   ou_state  NULL: no OU term.  Otherwise the caller's Ornstein-Uhlenbeck state [batch][act] float64 on the device, advanced once per query
 *         in the reference's order, float64, no fused multiply-add: s = s + (ou_theta (ou_mu - s) + ou_sigma n); then
 *         action = (float)((double)g + s) (numpy's float32 += float64).  mean and log_prob do not change.  The normals n ~ N(0, 1) come from
 *         Philox4x32-10 keyed by (seed, call_index, GLOBAL env id, unit) under a stream tag of their own (independent of the dropout masks
 *         and eps), so a split batch reproduces the whole batch bit for bit, whichever entry point runs the query.  Rows >= batch (ragged
 *         workgroups, padding) are not touched.
 * AOG_ERR_INVALID for a mode other than 0 / 1, a nonzero reserved0, a non-finite ou_mu / ou_theta / ou_sigma or ou_sigma < 0 (checked
 * before any device work).  The _noise entry points with noise = NULL are the plain ones; the plain ones forward to them with NULL. */
#define AOG_ACTION_SAMPLE 0
#define AOG_ACTION_MEAN 1
typedef struct aog_action_noise {
  int32_t mode;                         /* AOG_ACTION_SAMPLE or AOG_ACTION_MEAN */
  int32_t reserved0;                    /* = 0 */
  double* ou_state;                     /* [batch][act] float64 device pointer, nullable */
  double ou_mu, ou_theta, ou_sigma;     /* main.py:218-220: 0, 0.3, 0.05 */
} aog_action_noise;
int aog_actor_act_noise(const aog_actor* net, int device, const void* obs_dev, int obs_is_f16, float* mean_dev, float* action_dev, float* log_prob_dev,
                        const aog_action_noise* noise /* nullable */, void* stream);

/* ---- causal policy stepping (ABI 21): the rollout's actor.get_action(obs) -> env.step(action) (algorithm.py:256-262) with the policy
 * attached to the env.  The epilogue of step t, the policy query (aog_actor_act's arithmetic) on its float16 observation and the
 * action -> actuator prologue of step t + 1 run as ONE launch, 16 envs per workgroup: results bit-identical to aog_step + aog_actor_act
 * (obs_is_f16 = 1) + the next aog_step's prologue, log_prob up to the summation order aog_actor_act itself leaves open.
 *   net          batch = B, state_dim = obs_dim^2, act_dim = n_modes, and every check of aog_actor_act; else AOG_ERR_INVALID.  What does not fit
 *                the LDS beside the epilogue and prologue (state_dim 1024 fits up to hidden_dim 150 at least) is AOG_ERR_UNSUPPORTED, naming the sizes.
 *                net->call_index keys the query's random streams exactly as in aog_actor_act (a query consumes one index).
 *   obs          required (the query reads it); obs_raw nullable.
 *   action_out [B][A], log_prob_out [B] float32 required; mean_out [B][A] float32 nullable.
 * Between a call that leaves an action pending and the next aog_step_act the mirror already holds that action: aog_reset, aog_step,
 * aog_get_state, aog_get_actuators, aog_focal_image(s), aog_sh_* ... fail with AOG_ERR_STATE, as after aog_step_pipelined; aog_set_actuators
 * / aog_set_state replace the mirror and drop the pending action.  Works with aog_set_lookahead (the tail reads no screens; the next step's
 * extrusion is released before the epilogue as in aog_step).  A failure after the step counters moved makes the handle unusable, as in
 * aog_step.
 *
 * aog_reset with the policy attached: aog_reset of the whole batch (a masked reset goes through aog_reset), then the policy query on the reset
 * observation and the prologue of step 1 in the same launch as the reset's epilogue.  Leaves the first action pending. */
int aog_reset_act(aog_env* env, const aog_actor* net, float* obs_raw_dev, uint16_t* obs_dev, float* action_out, float* log_prob_out,
                  float* mean_out /* nullable */, void* stream);
/* Step t with the policy attached.  action = NULL: step the pending action (from aog_reset_act or the previous aog_step_act);
 * non-NULL: no action may be pending (the first step after a plain aog_reset); AOG_ERR_INVALID otherwise.  Unless this is the episode's
 * last step (cfg.max_steps steps after the last whole-batch reset), the tail queries the policy on obs_t, writes action / log_prob / mean of
 * step t + 1 and loads that action into the mirror (pending), *queried = 1; on the last step it is a plain epilogue, the policy outputs are
 * untouched and *queried = 0.  Other arguments as aog_step. */
int aog_step_act(aog_env* env, const aog_actor* net, const float* action_dev, float* obs_raw_dev, uint16_t* obs_dev, float* reward_dev,
                 uint8_t* done_dev, float* power_dev, float* strehl_dev, float* action_out, float* log_prob_out, float* mean_out,
                 int* queried /* host int, nullable */, void* stream);
/* aog_reset_act / aog_step_act with an action form (aog_action_noise above; NULL = the plain calls).  The fused tail applies it exactly as
 * aog_actor_act_noise does: the action it writes and loads into the mirror is the noisy / mean one, and the OU state advances once per query
 * (not on an episode's last step, which queries nothing). */
int aog_reset_act_noise(aog_env* env, const aog_actor* net, float* obs_raw_dev, uint16_t* obs_dev, float* action_out, float* log_prob_out,
                        float* mean_out /* nullable */, const aog_action_noise* noise /* nullable */, void* stream);
int aog_step_act_noise(aog_env* env, const aog_actor* net, const float* action_dev, float* obs_raw_dev, uint16_t* obs_dev, float* reward_dev,
                       uint8_t* done_dev, float* power_dev, float* strehl_dev, float* action_out, float* log_prob_out, float* mean_out,
                       int* queried /* host int, nullable */, const aog_action_noise* noise /* nullable */, void* stream);

/* ---- predictive linear controller: a per-env recursive-least-squares predictor learnt on the device (additive in ABI 22; no counterpart in
 * the reference) ----
 * The data-driven linear predictor learnt controllers are read against.  It depends on no sensor and on no aog_env: it is fed a
 * pseudo-open-loop measurement y_t [B][A] float64, the actuator vector (metres) that would have flattened the wavefront at step t —
 * aog_wavefront_truth's act_ideal, or aog_pyramid_update with gain = 1 — and returns its prediction of y_{t+1}.  Per env, n = act_dim x
 * order, everything float64 without fused multiply-add: W [n][A], P [n][n], a history of the last `order` measurements divided by
 * `scale` (the regressor x: newest measurement first), `count` (measurements taken) and `skipped`.  After create or reset: W = the
 * persistence predictor (rows 0 .. A - 1 the identity, the rest 0), P = p0 I, an empty history, both counters 0.
 *
 * One update of a selected env (mask_dev: nullable [B] uint8 device array, non-zero = selected), with c = count as the call finds it:
 *   1. if c >= order a previous regressor x_ exists:  e = y / scale - W' x_,  g = P x_,  d = forgetting + x_' g,
 *      W[i][j] += (g[i] / d) e[j],  P[i][j] = (P[i][j] - (g[i] g[j]) / d) / forgetting  (g[i] g[j] is formed first: P stays symmetric bit
 *      for bit; the blob handed to the set_state call must hold a symmetric P, as every blob of the get_state call does);
 *   2. y / scale is pushed into the history, count = c + 1;
 *   3. if c >= order (step 1 ran): pred = scale W' x with the new W and the new x; otherwise pred = y, the same bits (persistence).  So the
 *      first `order` predictions are the measurements themselves and the first prediction through W is made by a W that has learnt once;
 *   4. innov (nullable) = scale e, zero while no regressor exists.
 * An env whose row of y holds a non-finite value keeps its whole state; its pred row is a copy of its y row, its innov row zero, and
 * `skipped` counts it.  Envs the mask leaves out are touched nowhere, and neither are their rows of pred and innov.
 * One workgroup per env, every sum in an order fixed by (act_dim, order) alone (csrc/k_predictor.h): any split of a batch over handles
 * reproduces the whole batch bit for bit.  P and W are read once and written once per update up to n = 128 (16 n^2 + 16 n A bytes per env);
 * from n = 129 to the limit n = 256 they are read twice (24 n^2 + 24 n A).  Plain vector stores, no atomics, no host synchronisation.
 * AOG_ERR_INVALID, before any device work: batch < 1, act_dim outside [1, 256], order < 1, forgetting outside (0, 1], a non-finite or
 * non-positive p0 or scale, a nonzero reserved field.  AOG_ERR_UNSUPPORTED, naming the sizes: n > 256.  env_id_base is carried for the
 * caller (the global id of row 0) and enters no arithmetic.  The struct is six int32 and three doubles; it has no index in aog_struct_size. */
typedef struct aog_predictor aog_predictor;
typedef struct aog_predictor_config {
  int32_t batch, act_dim, order, env_id_base;
  int32_t reserved0, reserved1;         /* = 0 */
  double forgetting;                    /* lambda in (0, 1] */
  double p0;                            /* P = p0 I after create / reset */
  double scale;                         /* metres per unit of the regressor (BatchedAOEnv: wavelength_wfs / 2 pi) */
} aog_predictor_config;
int aog_predictor_create(const aog_predictor_config* cfg, int device, aog_predictor** out);
void aog_predictor_destroy(aog_predictor* p);
/* The selected envs (mask_dev as above) back to the state after create, `skipped` included.  Stream-ordered. */
int aog_predictor_reset(aog_predictor* p, const uint8_t* mask_dev, void* stream);
/* y_dev, pred_dev [B][A] float64 device pointers, innov_dev likewise or NULL.  Stream-ordered; pred_dev may be y_dev. */
int aog_predictor_update(aog_predictor* p, const double* y_dev, const uint8_t* mask_dev, double* pred_dev, double* innov_dev, void* stream);
/* Checkpointing: per env, one after the other, W [n][A], P [n][n], the history [n] (float64), count and skipped (int64) — so the blob of
 * a whole batch is the blobs of its parts in a row.  A handle of the same configuration that takes the blob resumes bit-identically. */
int64_t aog_predictor_state_bytes(const aog_predictor* p);
int aog_predictor_get_state(aog_predictor* p, void* blob_dev, void* stream);
int aog_predictor_set_state(aog_predictor* p, const void* blob_dev, void* stream);

/* ---- closed-loop modal telemetry: per-env rings of measurements, their power spectral densities and the optimised integrator gains
 * (additive in ABI 22; no counterpart in the reference) ----
 * Independent of any aog_env and of any sensor, like aog_predictor.  Per env: hist [length][act_dim] float64, a ring in which sample
 * number c lies in row c mod length; `count` (samples stored) and `skipped`, int64.  length T is a power of two in [64, 1024], act_dim A
 * in [1, 128].  Everything float64 without fused multiply-add, every sum in an order that (A, T, S) alone fix (csrc/k_telemetry.h): any
 * split of a batch over handles, and any mask, reproduces the whole batch bit for bit.  Plain vector stores, no atomics, no host
 * synchronisation; the calls on one handle are ordered by the one stream they are given.  mask_dev: nullable [B] uint8 device array,
 * non-zero = selected; envs it leaves out are touched nowhere, and neither are their rows of any output.
 *
 * aog_telemetry_push stores the row y [b] of every selected env at row count mod T and adds 1 to count; a row that holds a non-finite
 * value is not stored: `skipped` counts it and count stays.
 *
 * aog_telemetry_psd is Welch's estimate over what the ring holds.  `segment` S is a power of two with 32 <= S <= T, the hop S / 2.  With
 * n = min(count, T): segments = floor((n - S) / (S / 2)) + 1, the last one ends at the newest sample, they are summed oldest first.  Per
 * segment and mode: subtract the segment's mean, multiply by the periodic Hann window w_n = (1 - cos(2 pi n / S)) / 2,
 * X_k = sum_n w_n (y_n - mean) exp(-2 pi i k n / S), and Phi[k] = m_k (mean over the segments of |X_k|^2) / (S sum_n w_n^2), m_k = 1 at
 * k = 0 and k = S / 2 and 2 between: the variance per bin (S sum w^2 is taken as its exact value 3 S^2 / 8).  psd_dev [B][A][S/2+1]
 * float64, segments_dev (nullable) [B] int32.  An env with n < S gets NaN rows and 0 segments.  The ring is read once.
 *
 * aog_telemetry_gains computes the same Phi and from it, per env and mode, the gain of the integrator a <- a + g m that minimises
 *   J(g) = sum_{k=1}^{S/2} |R_k(g)|^2 Phi[k],   R_k(g) = 1 / (1 + g z^-d / (1 - z^-1)),   z = exp(2 pi i k / S),   d = delay in {1, 2, 3, 4}
 * over the n_grid <= 64 ascending candidates grid_host (a HOST array), each in (0, g_max(d)), g_max(d) = 2 sin(pi / (2 (2 d - 1))), the
 * stability limit of z^d - z^(d-1) + g = 0 (2 at d = 1, 1 at d = 2).  gain_dev [B][A] = the first minimiser in grid order, cost_dev
 * [B][A] its J, cost_all_dev (nullable) [B][A][n_grid] every J; NaN for an env with n < S.  |R_k(g)|^2 depends on (k, g) alone: it is
 * BUILT ON THE DEVICE once per call (k_telemetry_rk, float64, into a buffer of the handle), not uploaded.
 * AOG_ERR_INVALID, before any device work: batch < 1, act_dim outside [1, 128], a length or segment that is not such a power of two, a
 * delay outside [1, 4], n_grid outside [1, 64], a candidate outside (0, g_max(d)) or not above the one before it.  env_id_base is
 * carried for the caller and enters no arithmetic.  The struct is four int32; it has no index in aog_struct_size. */
typedef struct aog_telemetry aog_telemetry;
typedef struct aog_telemetry_config {
  int32_t batch, act_dim, length, env_id_base;
} aog_telemetry_config;
int aog_telemetry_create(const aog_telemetry_config* cfg, int device, aog_telemetry** out);
void aog_telemetry_destroy(aog_telemetry* t);
/* The selected envs back to the state after create: a ring of zeros, both counters 0.  Stream-ordered. */
int aog_telemetry_reset(aog_telemetry* t, const uint8_t* mask_dev, void* stream);
int aog_telemetry_push(aog_telemetry* t, const double* y_dev, const uint8_t* mask_dev, void* stream);
int aog_telemetry_psd(aog_telemetry* t, int segment, double* psd_dev, int32_t* segments_dev, const uint8_t* mask_dev, void* stream);
int aog_telemetry_gains(aog_telemetry* t, int segment, int delay, const double* grid_host, int n_grid, double* gain_dev, double* cost_dev,
                        double* cost_all_dev, const uint8_t* mask_dev, void* stream);
/* Checkpointing: per env, one after the other, hist [T][A] (float64), count and skipped (int64) — the blob of a whole batch is the blobs of
 * its parts in a row.  A handle of the same configuration that takes the blob resumes bit-identically. */
int64_t aog_telemetry_state_bytes(const aog_telemetry* t);
int aog_telemetry_get_state(aog_telemetry* t, void* blob_dev, void* stream);
int aog_telemetry_set_state(aog_telemetry* t, const void* blob_dev, void* stream);

/* ---- stochastic parallel gradient descent (SPGD): the sensorless baseline, as a controller on the device (additive in ABI 22; no
 * counterpart in the reference) ----
 * The one classical controller that sees only what a learnt policy sees: a scalar quality of the last command.  Two-sided SPGD with
 * Bernoulli perturbations, per env.  State: the centre command u [A] float64, the iteration k (uint32), the half h in {0, 1} and J_plus
 * (float64).  Per-env hyper-parameters gain [B] and amplitude [B] (float64, 0 until aog_spgd_set_params), one bound clip on |u_i| (0: none).
 *   delta_k in {-1, +1}^A: actuator i takes bit i & 31 of word (i >> 5) & 3 of the Philox4x32-10 call keyed by `seed` (low word, high word)
 *   with counter (env_id_base + env, k, i >> 7, 0x53504744); a set bit is +1.  Keyed by the GLOBAL env id: a split batch reproduces the whole.
 *   query, h = 0: the command in place gave the metric J:  J_plus = J,  emit u - amplitude delta_k,  h = 1;
 *   query, h = 1: u = clip(u + (gain (J_plus - J)) delta_k),  k = k + 1,  h = 0,  emit u + amplitude delta_k  (the new k's delta);
 *   reset of an env: u = 0 (or its row of act_dev),  h = 0,  k KEPT (no stream is replayed),  emit u + amplitude delta_k.
 * J is a float32 (what aog_step stores as power, Strehl or reward) widened to float64; every product and sum above is one rounded float64
 * operation in the order written, nothing fused; the emitted command is the float32 of the float64 sum, [B][A], raw actuators: the action
 * of an sh_operation handle.  A host replay from the recorded metrics is therefore bit-exact.  One wave per env, one Philox evaluation per
 * wave and 2048 actuators; plain vector stores, no atomics, no host synchronisation.  mask_dev: nullable [B] uint8 device array, non-zero =
 * selected; envs it leaves out are touched nowhere, and neither are their rows of action_out.
 * AOG_ERR_INVALID, before any device work: a wrong abi_version, num_envs < 1, act_dim < 1, a metric outside AOG_SPGD_*, a nonzero reserved
 * field, a NaN, infinite or negative clip, gain or amplitude.  The struct is four int32, a uint64, two int32 and a double; it has no index in
 * aog_struct_size. */
enum { AOG_SPGD_POWER = 0, AOG_SPGD_STREHL = 1, AOG_SPGD_REWARD = 2 };
typedef struct aog_spgd aog_spgd;
typedef struct aog_spgd_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, act_dim, env_id_base;
  uint64_t seed;
  int32_t metric;                       /* AOG_SPGD_*: which of the step's outputs aog_step_spgd descends on */
  int32_t reserved0;                    /* = 0 */
  double clip;                          /* bound on |u_i|; 0 = none */
} aog_spgd_config;
int aog_spgd_create(const aog_spgd_config* cfg, int device, aog_spgd** out);
void aog_spgd_destroy(aog_spgd* spgd);
/* gain_host, amplitude_host: HOST arrays [B].  Blocking copy. */
int aog_spgd_set_params(aog_spgd* spgd, const double* gain_host, const double* amplitude_host);
/* Reset of the selected envs.  act_dev: nullable [B][A] float64 device array to start u from (aog_get_actuators' form); action_out: nullable. */
int aog_spgd_reset(aog_spgd* spgd, const uint8_t* mask_dev, const double* act_dev, float* action_out, void* stream);
/* One query of the selected envs on metric_dev [B] float32. */
int aog_spgd_update(aog_spgd* spgd, const float* metric_dev, const uint8_t* mask_dev, float* action_out, void* stream);
/* Checkpointing: per env, one after the other, u [A] and J_plus (float64), then k and h (uint32) — the blob of a whole batch is the blobs
 * of its parts in a row.  A handle of the same configuration and parameters that takes the blob resumes bit-identically. */
int64_t aog_spgd_state_bytes(const aog_spgd* spgd);
int aog_spgd_get_state(aog_spgd* spgd, void* blob_dev, void* stream);
int aog_spgd_set_state(aog_spgd* spgd, const void* blob_dev, void* stream);
/* aog_reset_act / aog_step_act with the SPGD query in the policy's place (k_epilogue_spgd_prologue: the epilogue of step t, the query on
 * the metric it has just stored and the prologue of step t + 1 as one launch, 16 envs per workgroup).  Results bit-identical to aog_reset +
 * aog_spgd_reset (act_dev = the handle's actuators unless cfg.flat_mirror_start) resp. aog_step + aog_spgd_update on that step's output +
 * the next aog_step's prologue.  Argument rules, pending-action rules and the unusable-handle rule after a late failure as aog_reset_act /
 * aog_step_act; action_out [B][A] float32 required.  On the episode's last step aog_step_spgd is a plain epilogue: no query, action_out and
 * the controller untouched, *queried = 0.  The step's output that cfg.metric names may be NULL (the controller then keeps the metric in a
 * buffer of its own).  AOG_ERR_INVALID: a handle without cfg.sh_operation (its action is rescaled to a fixed surface rms, so a perturbation
 * amplitude means nothing there), act_dim != n_modes, num_envs != the handle's, another env_id_base or device. */
int aog_reset_spgd(aog_env* env, aog_spgd* spgd, float* obs_raw_dev, uint16_t* obs_dev, float* action_out, void* stream);
int aog_step_spgd(aog_env* env, aog_spgd* spgd, const float* action_dev, float* obs_raw_dev, uint16_t* obs_dev, float* reward_dev,
                  uint8_t* done_dev, float* power_dev, float* strehl_dev, float* action_out, int* queried /* host int, nullable */, void* stream);

/* ---- link telemetry: per-env rings of the fibre-coupled power, their fade statistics, histogram and bit-error rate (additive in ABI 22;
 * no counterpart in the reference) ----
 * Independent of any aog_env, like aog_telemetry.  Per env one record, which is also the checkpoint blob: ring [length] float32 (sample
 * number c lies at c mod length), then `count` (samples stored) and `skipped`, int64.  length T is a power of two in [64, 4096].  Plain
 * vector stores, no atomics on floats, no host synchronisation; the calls on one handle are ordered by the one stream they are given.
 * mask_dev: nullable [B] uint8 device array, non-zero = selected; envs it leaves out are touched nowhere, and neither are their rows of
 * any output.
 *
 * aog_link_push stores power_dev [b] (float32 [B] on the device: what a step writes as power) of every selected env at count mod T and
 * adds 1 to count; a non-finite sample is not stored: `skipped` counts it and count stays.
 *
 * aog_link_statistics works, per env, over its window: the last n = min(count, T) samples p_0 .. p_{n-1}, oldest first.  One launch covers
 * every env, threshold, bin and Q factor; the ring is read once.
 *   mean_dev, mean_square_dev [B] float64: sum p / n and sum p^2 / n, float64 sums of the float32 samples, each square exact in float64;
 *   minimum_dev, maximum_dev [B] float32, exact; samples_dev [B] int32 = n.
 *   Reference level P: the caller's `reference` (positive, finite) under AOG_LINK_REF_ABSOLUTE, the env's own mean under
 *   AOG_LINK_REF_MEAN (`reference` is then ignored); reference_dev [B] float64 receives it.
 *   Thresholds: n_edges = K <= 16 ascending positive factors edges_rel (a HOST array); the edge is the float64 product P f_k, sample i
 *   is in fade k when (double) p_i < P f_k.  below_dev, fades_dev, longest_dev [B][K] int32: the samples in fade, the maximal runs of
 *   consecutive in-fade samples (a run cut by either end of the window counts as one) and the longest run in frames.
 *   Histogram: n_hist = E <= 64 ascending positive factors hist_edges_rel (HOST) give hist_dev [B][E + 1] int32: bin 0 counts p < P g_0,
 *   bin j counts P g_{j-1} <= p < P g_j, bin E counts p >= P g_{E-1}; every row sums to n.
 *   Bit-error rate of on-off keying at the receiver Q factors q (HOST, n_q = Q <= 8, each positive and finite), at the reference level:
 *   ber_dev [B][Q] float64 = (1 / n) sum_i erfc(q_m p_i / (P sqrt 2)) / 2.
 *   An env with n = 0 gets 0 in every integer output and NaN in every float output.  K, E or Q may be 0; the outputs of a zero size
 *   may be NULL, all others are required.
 * Every float64 sum is taken in an order that (T, n) alone fix (csrc/k_link.h): any split of a batch over handles, and any mask,
 * reproduces the whole batch bit for bit.
 * AOG_ERR_INVALID, before any device work, with aog_last_error naming the field: a wrong abi_version, num_envs < 1, a length that is
 * not such a power of two, a nonzero reserved field; a reference_mode outside AOG_LINK_REF_*, an absolute reference that is not
 * positive and finite, K, E or Q beyond its limit, factors that are not positive, finite and strictly ascending, a q that is not
 * positive and finite.  env_id_base is carried for the caller and enters no arithmetic.  The struct is five int32; it has no index in
 * aog_struct_size. */
enum { AOG_LINK_REF_ABSOLUTE = 0, AOG_LINK_REF_MEAN = 1 };
enum { AOG_LINK_MAX_EDGES = 16, AOG_LINK_MAX_HIST = 64, AOG_LINK_MAX_Q = 8 };
typedef struct aog_link aog_link;
typedef struct aog_link_config {
  int32_t abi_version;                  /* = AOG_ABI_VERSION */
  int32_t num_envs, length, env_id_base;
  int32_t reserved;                     /* = 0 */
} aog_link_config;
int aog_link_create(const aog_link_config* cfg, int device, aog_link** out);
void aog_link_destroy(aog_link* link);
/* The selected envs back to the state after create: a ring of zeros, both counters 0.  Stream-ordered. */
int aog_link_reset(aog_link* link, const uint8_t* mask_dev, void* stream);
int aog_link_push(aog_link* link, const float* power_dev, const uint8_t* mask_dev, void* stream);
int aog_link_statistics(aog_link* link, int reference_mode, double reference, const double* edges_rel, int n_edges,
                        const double* hist_edges_rel, int n_hist, const double* q, int n_q, int32_t* samples_dev, double* mean_dev,
                        double* mean_square_dev, float* minimum_dev, float* maximum_dev, double* reference_dev, int32_t* below_dev,
                        int32_t* fades_dev, int32_t* longest_dev, int32_t* hist_dev, double* ber_dev, const uint8_t* mask_dev, void* stream);
/* Checkpointing: per env, one after the other, ring [T] (float32), count and skipped (int64) — the blob of a whole batch is the blobs of
 * its parts in a row.  A handle of the same configuration that takes the blob resumes bit-identically. */
int64_t aog_link_state_bytes(const aog_link* link);
int aog_link_get_state(aog_link* link, void* blob_dev, void* stream);
int aog_link_set_state(aog_link* link, const void* blob_dev, void* stream);

/* Self-test hook: sin(2 pi u), cos(2 pi u) for n float32 revolutions u_dev with the fused kernels' device code.
 * flavour 0 = polynomial, 1 = v_sin_f32/v_cos_f32 after the exact reduction, 2 = v_sin_f32/v_cos_f32 on raw input. */
int aog_selftest_sincos(const float* u_dev, float* sin_dev, float* cos_dev, int n, int flavour, void* stream);

/* Self-test hook: the Shack-Hartmann camera's photon noise (large_poisson, AO_env.py:272-275) on caller-supplied expected counts:
 * lam_dev / out_dev [n_env][n][n] float64, drawn by the same device code and Philox keying (env, row, column, call) as aog_sh_update(NULL) and the
 * fused row pass.  For distribution tests of the sampler (exact inversion below 12 counts, skew-corrected rounded normal above). */
int aog_selftest_poisson(const double* lam_dev, double* out_dev, int n_env, int n, uint64_t seed, uint32_t call, void* stream);

/* Self-test hook for the failure path of the dynamic atmosphere's inter-workgroup barrier (k_extrude16_split): runs the wind extrusion of
 * one step with one of every group's four workgroups absent and a short poll limit, so the partners' bounded wait gives up exactly as it
 * would if they were not co-resident.  Synchronises.  Afterwards aog_device_status() reports 1 and aog_step / aog_reset fail with
 * AOG_ERR_STATE until new screens are installed for the whole batch or a state is restored; the handle's screens are invalid (that is the
 * point).  Envs must move by at least one pixel in the step for a barrier to be reached.  AOG_ERR_UNSUPPORTED for handles that do not
 * use the split extrusion kernel. */
int aog_selftest_barrier_timeout(aog_env* env, void* stream);

/* Microseconds-resolution timing of the dominant (fused) kernel of the most recent aog_step/aog_reset calls,
 * measured with HIP events on the stream the kernel was launched on.  Enable, run steps, then read the
 * mean duration (ms) and the number of launches averaged.  enable = n > 1 times one block of consecutive launches (aog_profile_block, default 8) in n
 * only — the middle block of every n: the two event records
 * of a timed launch hold the stream for ~6 us, which a throughput measurement running at the same time should not pay on
 * every step. */
int aog_profile_enable(aog_env* env, int enable);
/* Launches per timed block (default 8; 1 .. 64): a window of a few dozen steps takes a short block so that the records stay ~1 % of it
 * (ABI 16).  Takes effect at the next aog_profile_enable / aog_profile_read. */
int aog_profile_block(aog_env* env, int launches);
int aog_profile_read(aog_env* env, double* mean_ms, int* launches);
/* While profiling is enabled the kernels that dominate the other workloads are timed the same way (HIP events on the launch stream,
 * every launch: they run once per reset or take >= 100 us): which = one of AOG_PROF_*; returns the mean duration and the number of launches
 * collected by the LAST aog_profile_read (which drains the events of every kernel).  AOG_PROF_FUSED repeats that call's own result. */
enum {
  AOG_PROF_FUSED = 0,        /* k_fused_tab / k_fused_valu / k_fused_ref                                   */
  AOG_PROF_SCREEN_ROWS = 1,  /* k_screen2_rows / k_screen_rows: spectrum draw + row transforms (K8 pass A) */
  AOG_PROF_SCREEN_COLS = 2,  /* k_screen2_cols / k_screen_cols (K8 pass B)                                 */
  AOG_PROF_PACK = 3,         /* k_screen_means + k_pack_tiles (or k_pack_screens) of a screen installation */
  AOG_PROF_EXTRUDE = 4,      /* k_extrude16_split / k_extrude16 / k_extrude (K7)                           */
  AOG_PROF_SH_FIELD = 5,     /* k_phase_mfma<FIELD> (K10)                                                  */
  AOG_PROF_SH_ROWS_FWD = 6,  /* k_sh_rows_fwd                                                              */
  AOG_PROF_SH_COLS = 7,      /* k_sh_cols                                                                  */
  AOG_PROF_SH_ROWS_INV = 8,  /* k_sh_rows_inv (+ photon noise + lenslet sums when fused)                   */
  AOG_PROF_COUNT = 9
};
int aog_profile_read_kernel(aog_env* env, int which, double* mean_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* AOGYM_H */
