// Internal (non-ABI) declarations shared by the translation units of libaogym.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/aogym.h"
#include "fused_layout.h"

namespace aog {
struct X8Table;
}

// Work buffers of a split-f16 Fraunhofer transform (K4, K11, the science camera, the pyramid) for a chunk of whole env tiles (mft_host.h:
// mft_work_alloc).  "Tiles", "natural" and "accumulator" in the comments of this file are DESIGN.md §5's ("Operand tiles of the MFT family"):
// a matrix [i][k] as [i >> 5][k >> 4] tiles of [4][64][8] f16, lane = i, K = k in one of the two orders; sizes are MftGeom's (mft_host.h).
struct MftWork {
  float* grid = nullptr;      // [chunk][Nyp][Nxp] reduced phases (revolutions), kShOutside outside the aperture and in the padding
  _Float16* T16 = nullptr;    // [chunk][Nxp / 32][v blocks][2] tiles: T' = m1' E, split, as pass 1's accumulators hold it (lane v, K = x accumulator)
  int chunk = 0;              // envs per round of phase grid + pass 1 + pass 2
};

struct aog_env {
  aog_config cfg{};
  int device = 0;
  bool tables_ready = false;
  bool screens_ready = false;
  int B = 0, Bp = 0, A = 0, A_pad = 0, n_ap = 0, n_ap_pad = 0, n_quads = 0, n_ptiles = 0, n_etiles = 0;
  int MRW = 0, MRS = 0;          // padded table counts of the fast kernels
  int MRW_used = 0, MRS_used = 0;
  int n_obs = 0, n_out = 0;
  int n_obs_tab = 0;             // observation outputs of the table route: n_obs, or 0 on the separable route (its n_out = the fiber modes)
  int kernel = AOG_KERNEL_VALU;  // resolved
  int sincos_hw = 0;
  aog::FusedGeom geom;           // launch geometry of the fused kernels (float64 validation handles: n_chunks = 1, the rest unused)
  int64_t dev_bytes = 0;
  // constant tables
  int32_t* ap_index = nullptr;
  std::vector<int32_t> ap_index_host;   // host copy (aog_upload_tables): ap_yx_table, the micro-lens table of aog_upload_sh
  uint32_t* ap_bits = nullptr;   // [N][ceil(N / 32)] the aperture as a bit mask (bit x & 31 of word x >> 5 of row y): k_screen2_cols' aperture sums
  double* syn_part = nullptr;    // [synthesis batch][column tiles] aperture sums of the screens just drawn, per column tile (k_screen2_cols -> k_mean_from_parts)
  size_t syn_part_elems = 0;
  float* modes_f32 = nullptr;    // [n_ap_pad][A_pad]
  _Float16* modes16 = nullptr;   // [n_ptiles][A_pad/16][hi|lo][64][8]
  float* tabs_f32 = nullptr;     // [n_ap_pad][TROW]
  _Float16* tab16 = nullptr;     // table-MFMA form: [n_ptiles][step 2][hi|lo][lane 64][8] A operands of the wfs tables
  float* sci_tile = nullptr;     // [n_ptiles][h 2][16] science table in accumulator order
  double* gram = nullptr;        // [A][A]
  double* wfs_coef = nullptr;    // [n_out][MRW_used][2]
  double* sci_coef = nullptr;    // [MRS_used][2]
  double* modes64 = nullptr;     // validation: [n_ap][A]
  double* tabs64 = nullptr;      // validation: [n_ap][MRW_used+MRS_used]
  // Shack-Hartmann chain (K10)
  bool sh_ready = false;
  int sh_n_sub = 0;
  int32_t* sh_slot = nullptr;
  double* sh_centres = nullptr;
  double* sh_ref = nullptr;
  double* sh_recon = nullptr;
  double* sh_mla = nullptr;       // [N*N] complex
  double* sh_tf = nullptr;        // [2N][2N] complex
  double* sh_xdet = nullptr;
  double* sh_act = nullptr;       // [B][A] deformable_mirror_shack.actuators
  _Float16* sh_act16 = nullptr;   // same, B-operand layout
  float* sh_phase = nullptr;      // psi_tile layout: wfs phase (rev) through the shack mirror
  void* sh_pad = nullptr;         // [B][2N][2N] complex work buffer (complex64, or complex128 when sh_double)
  void* sh_in = nullptr;          // [B][2N][2N] zero-padded forward input (padding never written)
  float* sh_tf32 = nullptr;       // [2N][2N] complex64 copy of the transfer function
  bool sh_double = false;         // complex128 transforms (aog_sh_tables.fft_double)
  double* sh_image = nullptr;     // [B][N*N]
  double* sh_noisy = nullptr;     // [B][N*N]
  void* sh_plan = nullptr;        // hipfftHandle (Z2Z, batch B)
  int sh_pruned = 0;              // L / 64 (4, 8, 16) when the pruned three-pass propagation is used (complex64, N = 128 / 256 / 512); 0 = hipFFT 2-D
  float* sh_tw = nullptr;         // [L] complex64 e^{+2 pi i j / L}
  int32_t* sh_ap_yx = nullptr;    // [n_ap] iy << 16 | ix of aperture pixel p
  float* sh_mla32 = nullptr;      // [N*N] complex64 micro-lens phase factor
  float* sh_ftab = nullptr;       // [n_ap] argument of the micro-lens factor in revolutions per packed aperture pixel (pruned route)
  double* sh_sums = nullptr;      // [B][n_sub][3] noisy per-lenslet sums of the fused row pass (aog_sh_image without an image pointer)
  bool sh_sums_ready = false;     // set by that call, consumed by the next aog_sh_update(null)
  float* sh_tfq = nullptr;        // [L / BC][64][64] complex64 transfer function in the column pass's lane / register order
  int sh_sep_rl = 0;              // RL of the separable two-pass propagation (transfer function = hx(kx) hy(ky)); 0 = three-pass form
  float* sh_hxq = nullptr;        // [LW][64] complex64 hx[lane / BC + RL k2]   (pass 1, layout B)
  float* sh_hyq = nullptr;        // [RL][64] complex64 hy[lane + LW r]         (pass 2, layout A)
  double sh_amp = 0, sh_scale = 0, sh_gain = 0, sh_leak = 0;
  uint32_t sh_calls = 0;
  // aog_sh_gradient (shack_gradient.hip): the call's own scratch, made on its first use
  _Float16* shg_act16 = nullptr;     // the point of evaluation, B-operand layout
  float* shg_phase = nullptr;        // psi_tile layout (generic route)
  double* shg_image = nullptr;       // [B][N*N] the clean image
  double* shg_coef = nullptr;        // [B][n_sub][4]: g_sx / F, g_sy / F, c_x, c_y
  double* shg_gscale = nullptr;      // [B] the divisor taken off the cotangent (a power of two)
  double* shg_qscale = nullptr;      // [B] and the one taken off the q grid
  float* shg_qgrid = nullptr;        // [B][N][N] q on the pupil grid (separable route)
  double* shg_q64 = nullptr;         // [B][n_ap] q per packed aperture pixel (generic route)
  double* shg_slabs = nullptr;       // [pixel chunk][A_pad][Bp] (separable) or [A][Bp] (generic)
  int32_t* shg_slot_start = nullptr; // [n_sub + 1] the pixels of the selected lenslets, lenslet by lenslet in raster order
  int32_t* shg_slot_pix = nullptr;
  void* shg_in = nullptr;            // generic route on a pruned handle: its own padded input, work array, float transfer function and plan
  void* shg_pad = nullptr;
  float* shg_tf32 = nullptr;
  void* shg_plan = nullptr;
  // device screen synthesis (K8)
  void* fft_plan = nullptr;      // hipfftHandle
  int fft_m = 0, fft_batch = 0;
  float* fft_work = nullptr;     // [fft_batch][m][m] complex64
  float* fft_crop = nullptr;     // [fft_batch][N][N]
  float* syn_T = nullptr;        // pruned synthesis: [syn_batch][m][N] complex64 (lines after pass A)
  float* syn_out = nullptr;      // [syn_batch][N][N]
  int syn_batch = 0, syn_m = 0;     // syn_m: q N of the literal layout, -(q N) of the two-band layout
  int screen_method = AOG_SCREENS_TWOBAND;
  float* low_c = nullptr;        // general route of the two-band form: low-band spectrum [fft_batch][KL][2 KL] complex64
  float* low_T = nullptr;        // and its lines [fft_batch][KL][N] complex64
  int low_key = 0;
  uint32_t* screen_gen = nullptr;   // [B] screens synthesised so far per env (Philox stream position of k_screen_rows / k_spectrum_fill)
  // focal-image export (optional)
  int n_focal = 0;
  double* focal_m1 = nullptr;    // [n_focal][N] complex
  double* focal_m2 = nullptr;    // [N][n_focal] complex
  double* focal_E = nullptr;     // [N][N] complex scratch
  double* focal_T = nullptr;     // [n_focal][N] complex scratch
  _Float16* focal_m1s = nullptr; // the batched matrix-core path (aog_focal_images): m1 2^e1, [nfp / 32][Nyp / 16] tiles, lane v, K = y natural
  _Float16* focal_m2s = nullptr; // m2 2^e2, [nfp / 32][Nxp / 16] tiles, lane u, K = x accumulator
  float focal_unscale = 1.f;     // 2^-(e1 + e2)
  int32_t* focal_ap_yx = nullptr;  // [n_ap] iy << 16 | ix of aperture pixel p (K4, K11 and the science camera: whoever comes first uploads it)
  MftWork focal_work;            // allocated by the first aog_focal_images; Nxp = N rounded up to 128, nfp / 32 v blocks
  _Float16* focal_act_ll = nullptr;  // [n_etiles][A_pad / 16][64][8] third f16 term of the actuators (K4 phases)
  // separable observation route (cfg.obs_separable, aog_upload_obs_mft; K11, k_obs.h)
  bool obs_sep = false;
  bool obs_ready = false;        // aog_upload_obs_mft done
  _Float16* obs_m1s = nullptr;   // m1 2^e1, K4's m1s layout with one v block
  _Float16* obs_m2s = nullptr;   // m2 2^e2, K4's m2s layout with one u block
  float obs_unscale = 1.f;
  MftWork obs_work;              // Nxp = N rounded up to 32, one v block
  _Float16* obs_act16 = nullptr; // actuators of the step being observed in the phase kernel's operand layouts (hi | lo, third term):
  _Float16* obs_act_ll = nullptr;//   their own buffers, so that nothing the fused kernel or a pipelined prologue reads is touched
  double* obs_pw = nullptr;      // [B][o^2] float64 powers of the last observation (the SSIM reward reads them)
  double* obs_m1d = nullptr;     // float64 handles: m1 [o][N], m2 [N][o] complex, E [N][N], T [o][N], F [B][o^2] complex
  double* obs_m2d = nullptr;
  double* obs_E = nullptr;
  double* obs_T = nullptr;
  double* obs_F = nullptr;
  // The off-step instruments below (wavefront fit, output gradient, science camera, pyramid sensor and its gradient) read the mirror through one
  // scratch pair (instrument_operands): the calls on a handle are ordered by their one stream and each rewrites the pair in full before it
  // reads it, so nothing is carried from one call to the next.  Made on first need, inst_act_ll only once a call asks for the third term.
  _Float16* inst_act16 = nullptr;  // the call's own copy of the actuators (or of its act_src) in act16's layout
  _Float16* inst_act_ll = nullptr; // and their third f16 term, in focal_act_ll's layout
  // wavefront fit (aog_upload_wavefront_fit, aog_wavefront_truth; wavefront.hip).  Nothing here is read or written by a reset or step.
  bool wf_ready = false;         // the fit is uploaded (aog_upload_tables clears it)
  double* wf_fit = nullptr;      // [A][A] P = pinv(Mc' Mc)
  double* wf_colsum = nullptr;   // [A] column sums of the mode matrix over the aperture
  _Float16* wf_tab16 = nullptr;  // modes as table operands: [n_ptiles][A_pad rows in blocks of 32][step 2][hi|lo][lane 64][8] (tab16's pixel order)
  double* wf_slabs = nullptr;    // [pixel chunk][A_pad + 2][Bp] partial sums, allocated by the first call
  double* wf_w = nullptr;        // float64 handles: [B][n_ap] path error of the call, allocated by the first call
  // wavefront projection onto a caller's shapes (aog_upload_wavefront_shapes, aog_wavefront_project; tomography.hip).  Off the step path like
  // the block above; float64 handles share wf_w with it (each call rewrites it in full before it reads it).
  bool tomo_ready = false;       // shapes are uploaded (aog_upload_tables clears it)
  int tomo_K = 0, tomo_gblk = 0, tomo_groups = 0;   // shapes; 32-row blocks per row group; row groups (fast handles)
  double tomo_unscale = 1.0;     // 1 / (the upload's operand scale x kActScale)
  _Float16* tomo_tab16 = nullptr;   // [group][n_ptiles][tomo_gblk blocks of 32 rows][step 2][hi|lo][lane 64][8]: pack_tab16_rows per group
  double* tomo_shapes64 = nullptr;  // float64 handles: [n_ap][K]
  double* tomo_rowsum = nullptr;    // [K] sum_p S[k][p]
  double* tomo_slabs = nullptr;     // [group][pixel chunk][32 tomo_gblk + 1][Bp] (float64 handles: [K + 1][Bp]); the last row is sum u
  // output gradient (aog_upload_gradient, aog_output_gradient; gradient.hip).  Nothing here is read or written by a reset or step.
  bool grad_ready = false;         // the gradient's tables are uploaded (aog_upload_tables clears it)
  float grad_tscale = 1.f;         // power of two the table operands are scaled by
  _Float16* grad_ftab16 = nullptr; // wfs tables as A operands of the forward sums: [n_ptiles][step 2][hi|lo][64][8] (tab16's order, 32 table rows)
  _Float16* grad_ttab16 = nullptr; // the same tables transposed (32 pixel rows, K = 32 tables): [n_ptiles][step 2][hi|lo][64][8]
  _Float16* grad_mtab16 = nullptr; // modes as table operands (wf_tab16's recipe)
  double* grad_stab = nullptr;     // [n_ptiles][h 2][16] science table in accumulator order
  _Float16* grad_cop16 = nullptr;  // [n_etiles][step 2][re|im][hi|lo][64][8] C of every env as B operands
  float* grad_csci = nullptr;      // [Bp][2] the science arm's C
  double* grad_fslabs = nullptr;   // forward partial sums [pixel chunk][rows][Bp], allocated by the first call (as the four below)
  double* grad_bslabs = nullptr;   // backward partial sums [pixel chunk][A rows][Bp]
  double* grad_cbuf = nullptr;     // [B][tables][2] C / cscale
  double* grad_cscale = nullptr;   // [B]
  double* grad_trig = nullptr;     // float64 handles: [B][n_ap][4]
  // observation gradient of the separable route (aog_upload_gradient_obs; gradient_obs.hip, k_gradient_obs.h).  Off the step path like the
  // block above; the phase grid and T' of a call go through obs_work, which every step rewrites in full before it reads it.
  bool gobs_ready = false;         // the transposed operand tables are uploaded (aog_upload_tables clears it)
  int gobs_chunk = 0;              // envs per round: obs_work.chunk, or less through AOG_GRAD_OBS_CHUNK (whole env tiles)
  double gobs_unscale = 1.0;       // 2^-(e1 + e2) of the two tables below
  _Float16* gobs_m1t = nullptr;    // m1' 2^e1 as A operands: [ceil(Nyp / 32)][2] tiles, lane y, K = v accumulator
  _Float16* gobs_m2t = nullptr;    // m2' 2^e2 as B operands: [Nxp / 32][2] tiles, lane x, K = u natural
  _Float16* gobs_wop = nullptr;    // [chunk][step 2][4][64][8] W / wscale of every env as A operands (row v, K = u)
  double* gobs_wscale = nullptr;   // [B] the power of two W was divided by
  double* gobs_slabs = nullptr;    // [pixel chunk][A rows][Bp] partial sums of the modes contraction of the observation's q
  double* gobs_m1td = nullptr;     // float64 handles: m1' [N][o], m2' [o][N] complex, F / W [o^2], P [N][o], H [N][N] complex, q [n_ap]
  double* gobs_m2td = nullptr;
  double* gobs_F = nullptr;
  double* gobs_W = nullptr;
  double* gobs_P = nullptr;
  double* gobs_H = nullptr;
  double* gobs_q = nullptr;
  // science camera (aog_upload_science, aog_science_*; science.hip).  Nothing here is read or written by a reset or step, and none of it
  // is part of the aog_get_state blob: the exposure is measurement data, and aog_set_state leaves sci_exposure / sci_frames as they were.
  bool sci_ready = false;        // the camera is uploaded (aog_upload_tables clears it)
  int sci_w = 0, sci_n_ee = 0;   // window side, number of encircled-energy radii
  double sci_ratio = 0, sci_peak = 0;   // lambda_wfs / lambda_sci; the unaberrated peak's share of the beam's power
  float sci_unscale = 1.f;       // 2^-(e1 + e2) of the operand tables
  _Float16* sci_m1s = nullptr;   // K4's m1s layout with ceil(w / 32) v blocks
  _Float16* sci_m2s = nullptr;   // K4's m2s layout with ceil(w / 32) u blocks
  MftWork sci_work;              // phases at the science wavelength; Nxp = N rounded up to 128, ceil(w / 32) v blocks
  double* sci_m1d = nullptr;     // float64 handles: m1 [w][N], m2 [N][w] complex, E [N][N], T [w][N], F [w][w] complex
  double* sci_m2d = nullptr;
  double* sci_E = nullptr;
  double* sci_T = nullptr;
  double* sci_F = nullptr;
  int32_t* sci_bin = nullptr;    // [w][w] radial bin of each pixel of the window (-1: outside every radius)
  double* sci_exposure = nullptr;   // [B][w][w] sum of the integrated frames
  int32_t* sci_frames = nullptr;    // [B] frames integrated
  // pyramid wavefront sensor (aog_upload_pyramid, aog_pyramid_*; pyramid.hip).  Nothing here is read or written by a reset or step, and of
  // all of it only pyr_frame travels with the aog_get_state blob (in its tail).  Every buffer is allocated by aog_upload_pyramid /
  // aog_upload_pyramid_reconstructor.
  bool pyr_ready = false;        // the sensor is uploaded (aog_upload_tables clears it)
  bool pyr_rec_ready = false;    // and its reconstructor
  int pyr_wq = 0, pyr_ns = 0, pyr_nmod = 0, pyr_nvalid = 0;   // samples per quadrant side, detector pixels per side, modulation points, valid pixels
  double pyr_photons = 0;        // photo-electrons per unit of frame value (0: no photon noise)
  uint64_t pyr_frame = 0;        // sensor calls since the upload (or what aog_set_state restored): the frame of the photon stream's counter
  float pyr_unscale = 1.f;       // what undoes the powers of two of m1s x m2s
  double pyr_back_unscale = 1.0; // and of the stored field x b1s x b2s
  _Float16* pyr_m1s = nullptr;   // [n_mod] x the science camera's m1s layout with ceil(w / 32) v blocks
  _Float16* pyr_m2s = nullptr;   // [n_mod] x its m2s layout
  _Float16* pyr_b1s = nullptr;   // [2][ceil(n_s / 32)][2 ceil(w / 32)] tiles: lane y', K = v accumulator
  _Float16* pyr_b2s = nullptr;   // [2][ceil(n_s / 32)][2 ceil(w / 32)] tiles: lane x', K = u accumulator
  MftWork pyr_work;              // phases at lambda_wfs; Nxp = N rounded up to 128, ceil(w / 32) v blocks
  _Float16* pyr_fop = nullptr;   // [chunk][nvb][2 nvb] tiles: F_j 2^6, split, k_pyr_back's A operands (lane u, K = v accumulator)
  float* pyr_tile_keep = nullptr;  // dynamic handles whose psi_tile a sensor call refreshes (obs_tiles): psi_tile as the call found it, put back behind the call
  double* pyr_m1d = nullptr;     // float64 handles: the four tables, E [N][N], T [w][N], F [w][w], X [2][n_s][w], G [4][n_s][n_s] complex
  double* pyr_m2d = nullptr;
  double* pyr_b1d = nullptr;
  double* pyr_b2d = nullptr;
  double* pyr_E = nullptr;
  double* pyr_T = nullptr;
  double* pyr_F = nullptr;
  double* pyr_X = nullptr;
  double* pyr_G = nullptr;
  int32_t* pyr_valid = nullptr;  // [n_valid] y n_s + x of the valid pixels
  double* pyr_acc = nullptr;     // [B][4][n_s][n_s] sum over the modulation points of the call in flight
  double* pyr_slopes = nullptr;  // [B][2 n_valid] slopes of the last aog_pyramid_update
  double* pyr_recon = nullptr;   // [A][2 n_valid]
  double* pyr_ref = nullptr;     // [2 n_valid]
  // its gradient (aog_pyramid_gradient; pyramid_grad.hip).  Every buffer is allocated by the first gradient call and given back by
  // aog_upload_pyramid; float64 handles only so far.
  double* pyg_gpix = nullptr;    // [B][4][n_s][n_s] the cotangent on the frame (g_frames + the slopes cotangent pulled back)
  double* pyg_m1t = nullptr;     // [n_mod] x m1_j' [N][w], m2_j' [w][N] complex
  double* pyg_m2t = nullptr;
  double* pyg_b1t = nullptr;     // [w][2 n_s] complex: column (s_y, y') of row v = b1[s_y][y'][v]
  double* pyg_b2t = nullptr;     // [2 n_s][w] complex: row (s_x, x') = b2[s_x][u][x'] over u
  double* pyg_W = nullptr;       // [s_y 2][n_s][s_x 2][n_s] complex: W of the four quadrants, rows of one s_y side by side
  double* pyg_Y = nullptr;       // [s_y 2][n_s][w] complex: W b2'
  double* pyg_V = nullptr;       // [w][w] complex
  double* pyg_P = nullptr;       // [N][w] complex: m1' V
  double* pyg_H = nullptr;       // [N][N] complex
  double* pyg_q = nullptr;       // [n_ap] the sum over the modulation points of 2 Re(i E H)
  double* pyg_slabs = nullptr;   // [A][Bp] sum_p M_pk q_p (fast handles: [pixel chunk][A_pad][Bp])
  double* pyg_gscale = nullptr;  // [B] the power of two of the largest |cotangent| of the env (1 for a zero cotangent)
  // fast handles: the transposed operand tables (made from the uploaded ones by the first call) and the chunk's work buffers
  _Float16* pyg_m1s_t = nullptr; // [n_mod][ceil(Nyp / 32)][2 nvb] tiles: lane y, K = v accumulator
  _Float16* pyg_m2s_t = nullptr; // [n_mod][Nxp / 32][2 nvb] tiles: lane x, K = u natural
  _Float16* pyg_b1s_t = nullptr; // [2][nvb][2 nsb] tiles: lane v, K = y' accumulator
  _Float16* pyg_b2s_t = nullptr; // [2][nvb][2 nsb] tiles: lane u, K = x' accumulator
  _Float16* pyg_vop = nullptr;   // [chunk][nvb][2 nvb] tiles: V_j / scales as A operands (lane v, K = u natural); the pads stay zero
  double* pyg_wscale = nullptr;  // [chunk] W's power of two over V's, of the modulation point in flight
  double* pyg_qscale = nullptr;  // [B] the power of two the env's q grid was divided by
  float* pyg_qgrid = nullptr;    // [chunk][Nyp][Nxp] q summed over the modulation points, on aperture pixels
  // state
  float* psi_rev = nullptr;     // [n_quads][Bp][4]  (handles that run the VALU kernel only)
  double* pack_mean = nullptr;   // [B] aperture means of the screens being installed (k_screen_means -> k_pack_tiles)
  double* layer_mean = nullptr;  // [B] aperture means of the layer sum being installed (aog_install_layer_sum: k_layer_mean -> k_layer_sum_*), allocated by the first call
  double* dist_basis = nullptr;  // [dist_terms][n_ap] pupil shapes of the modal disturbance in the masters' unit (aog_upload_disturbance_basis; aog_install_layer_sum_disturbed reads them)
  int dist_terms = 0;
  // sightline installation (aog_install_layer_sum_sightline): the shifts of the last one, [sight_layers][B][2] (sx, sy) in pixels; a
  // finite-range installation (aog_install_layer_sum_cone) keeps [sight_layers][B][3] (sx, sy, m) in the same buffers
  double* sight_shift = nullptr;   // device, room for 8 layers x 3; the kernels read it through SightLayers / ConeLayers
  double* sight_stage = nullptr;   // pinned, the same values: what a new installation's shifts are compared with and copied from
  hipEvent_t sight_ev = nullptr;   // recorded after the last copy out of the staging buffer
  int sight_layers = 0;            // layers the two buffers hold values for (0: none yet)
  int sight_width = 2;             // values per layer and env they hold: 2 (shifts) or 3 (shifts and magnification)
  float* psi_tile = nullptr;   // [Bp/32][n_ptiles][4][64][4]
  double* psi64 = nullptr;       // validation: [B][n_ap]
  double* act_dm = nullptr;      // [B][A]
  float* act_rev = nullptr;      // [A_pad][Bp]
  _Float16* act16 = nullptr;     // [Bp/32][A_pad/16][hi|lo][64][8]
  int32_t* t_render = nullptr;   // [B]
  // The observation a reset returns, kept between episodes (reset_impl): on a handle whose screens stay (not atm_dynamic), with a flat mirror
  // start, the table route and no detector, it is the same bits every episode until screens, tables or a state are installed.  Every such
  // installation clears reset_obs_valid; the next unmasked reset runs the pupil pass again and refills.
  bool reset_cache = true;       // AOG_RESET_CACHE=0 at aog_create: every reset runs the pupil pass (speed only, never results)
  bool reset_obs_valid = false;
  float* reset_obs_raw = nullptr;   // [B][n_obs] fp32, allocated by the first fill
  uint16_t* reset_obs = nullptr;    // [B][n_obs] f16 bits
  // dynamic atmosphere (cfg.atm_dynamic)
  bool layer_ready = false;
  // ring-direct form (fast MFMA handles): the fused kernel reads the fp32 ring copy of the master screens itself, no per-step repack
  bool ring_direct = false;
  bool tiles_stale = false;      // psi_tile (used by the focal-field / Shack-Hartmann / phase-screen paths) is older than the master screens
  float* psi_ring = nullptr;     // [B][N][N + 4] fp32, see aog::DynPsi
  uint32_t* quad_desc = nullptr; // [n_ptiles * 2][4]
  uint32_t* quad_cont = nullptr; // [n_ptiles * 2][4]
  unsigned* ext_bar = nullptr;   // group-barrier tickets of k_extrude16_split: two sets that alternate between steps (each launch zeroes the other set)
  int ext_bar_phase = 0;
  int* dev_status = nullptr;     // sticky device-side error word (1 = a bounded spin timed out)
  int* host_flag = nullptr;      // the same flag in pinned, device-mapped host memory: read by the host without a synchronisation
  int* host_flag_dev = nullptr;  // its device address
  int n_ext_groups = 0;
  int ext_resident = 0;          // workgroups of k_extrude16_split one launch may hold (occupancy query x CUs; 0 = not asked yet)
  unsigned ext_spin_limit = 1u << 24;   // polls before a barrier wait gives up (seconds)
  int ext_absent_part = -1;      // aog_selftest_barrier_timeout: the part that never arrives
  int32_t* ext_perm = nullptr;   // [n_ext_groups * 16] group slot -> env id, -1 = padding (envs sorted by wind, see aog_set_wind)
  double max_wind = 0;           // max |component| of any env's velocity (bounds the rounds per step)
  long long timestep = 0;        // AOEnv.timestep: monotone over episodes (AO_env.py:123)
  // lookahead (aog_set_lookahead): the wind extrusion of step t + 1 is launched by aog_step(t) on a stream of the library's own, behind
  // the fused kernel of step t, and runs beside the step's epilogue and whatever the caller does before aog_step(t + 1) (its policy query)
  bool lookahead = false;
  bool pre_evolved = false;      // the master screens / ring already stand at timestep + 1
  long long steps_since_reset = 0;   // steps since the last whole-batch aog_reset (lock-step episodes end at cfg.max_steps)
  hipStream_t ext_stream = nullptr;
  hipEvent_t ev_fused_done = nullptr, ev_ext_done = nullptr;
  double* psi_master = nullptr;  // [B][N*N] float64 toroidal screens
  int32_t* origin = nullptr;     // [B][2]
  uint32_t* ext_counter = nullptr;  // [B]
  double* velocity = nullptr;    // [B][2]
  double* psi_offset = nullptr;  // [B] piston offset used by the per-step repack
  double* psi_sum = nullptr;     // [B] aperture sums accumulated by the last repack
  int32_t* stencil_v = nullptr;
  int32_t* stencil_h = nullptr;
  int32_t* stencil_v_yx = nullptr;  // (sy << 16 | sx)
  int32_t* stencil_h_yx = nullptr;
  double* At_v = nullptr;        // [nz_v][N]
  double* Bt_v = nullptr;        // [N][N]
  double* At_h = nullptr;
  double* Bt_h = nullptr;
  double* Wa_v = nullptr;        // MFMA-blocked copies [row block][k/8][lane][2] (k_extrude16_split)
  double* Wb_v = nullptr;
  double* Wa_h = nullptr;
  double* Wb_h = nullptr;
  int nz_v = 0, nz_h = 0;
  // int8 composite extrusion (aog_upload_layer_composite; kernels in k_extrude_i8.h).  x8_host: host copies of the operator tables (opaque here)
  void* x8_host = nullptr;
  aog::X8Table* x8_tables_dev = nullptr;   // [2][kX8MaxK + 1]
  int x8_kmax[2] = {0, 0};         // k_max uploaded per axis (0 = none)
  int ext_mode = 0;                // AOG_EXTRUDE_*
  int32_t* x8_dxy = nullptr;
  int32_t* x8_slot = nullptr;
  int32_t* x8_list = nullptr;
  int32_t* x8_tile_k = nullptr;
  int32_t* x8_items = nullptr;
  int8_t* x8_Z8 = nullptr;
  double* x8_rec = nullptr;
  double* x8_colbuf = nullptr;
  hipStream_t x8_plan_stream = nullptr;   // the plan of step t + 1 runs here beside step t's fused kernel (x8_evolve)
  hipEvent_t x8_ev_evolved = nullptr, x8_ev_planned = nullptr;
  int x8_ahead_level = 0;                 // what was made ahead for x8_plan_step: 1 the plan, 2 the plan and the x phase
  long long x8_plan_step = -1;            // step the arrays of k_x8_plan were last made for ahead of time (-1 none, -2 dropped)
  int x8_tiles64_max = 0, x8_slots_max = 0, x8_KsTot_max = 0, x8_rt_max = 0, x8_items_max = 0;
  int near_v = 0, near_h = 0;    // stencil samples in the two newest slices come first in the uploaded order (aog_upload_layer)
  double sqrt_cn2 = 0, pitch = 0, delta_t = 0;
  // per-env turbulence strength (aog_set_turbulence).  turb_cn2 empty = every env at the handle-wide value (sqrt_cn2, the cn_squared of
  // aog_generate_screens).  The device arrays are derived on the host and copied from pinned staging; the screen amplitudes depend on the
  // generation arguments too and are refreshed by aog_generate_screens when those or the values change (turb_amp_key)
  std::vector<double> turb_cn2;  // [B] host copy
  double* turb_f64 = nullptr;    // [2][B] device: sqrt(Cn^2_e) (float64 extrusion), c_e = sqrt(Cn^2_e) / sqrt_cn2 <= 1 (int8 extrusion)
  float* turb_f32 = nullptr;     // [3][B] device: two-band ampH, ampL; literal crop scale
  double* turb_stage64 = nullptr;   // pinned [2][B]
  float* turb_stage32 = nullptr;    // pinned [3][B]
  hipEvent_t turb_ev64 = nullptr, turb_ev32 = nullptr;   // recorded after the last copy out of each staging buffer
  long long turb_version = 0;    // bumped by every aog_set_turbulence with values
  long long turb_amp_key[3] = {-1, 0, 0};   // (version, oversampling, pixel pitch bits) turb_f32 was made for
  // photodetector model of the observations (aog_set_detector).  det_on = false: the noise-free kernels with their arguments, as before
  bool det_on = false;
  double* det_par = nullptr;     // [3][B] device: photons per frame, read noise, background
  double* det_stage = nullptr;   // pinned [3][B]
  hipEvent_t det_ev = nullptr;   // recorded after the last copy out of the staging buffer
  uint64_t obs_frame = 0;        // observations written so far (each aog_reset* / aog_step* call adds one): the frame of the detector's counter
  const double* next_noise = nullptr;
  int next_noise_max_ext = 0;
  unsigned long long rng_seed = 1234;
  double* partials = nullptr;
  size_t partial_elems = 0;
  // profiling of the fused kernel
  float* ret_acc = nullptr;      // caller-owned episode-return accumulator (aog_set_return_accumulator)
  bool profile = false;
  bool pro_pending = false;      // aog_step_pipelined: the actuators already hold the NEXT step's action (its prologue rode with the last epilogue)
  int profile_block = 8;         // launches per timed block (aog_profile_block)
  int profile_every = 1;         // time every n-th launch of the fused kernel (aog_profile_enable(env, n))
  unsigned profile_phase = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<int> event_kernel;    // AOG_PROF_* id of each used event pair
  size_t events_used = 0;
  double prof_ms[AOG_PROF_COUNT] = {};   // totals of the last aog_profile_read, per kernel id
  int prof_n[AOG_PROF_COUNT] = {};
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;   // size of allocs[i] (dev_release gives work buffers back before the handle is destroyed)
};

namespace aog_host {
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the FUNCTION (per device), not to a handle: remember the largest request
// made for each (function, device) in this process and only ever raise it, so that handles of different shapes coexist.
int ensure_dynamic_lds(const void* fn, size_t bytes, int device);
#ifdef AOG_DEV
extern long long* dev_timeline;   // per-wave time stamps of the last fused launch (AOG_DEV_TIMELINE=1)
#endif
}  // namespace aog_host
