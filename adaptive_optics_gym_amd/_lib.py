"""ctypes binding of ``libaogym.so`` (the C-ABI declared in ``include/aogym.h``).

There is no CPU fallback: if the shared library is missing the import of the env classes still works (so
CPU-only tooling can inspect them) but the first call raises ``RuntimeError`` naming the build command.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaogym.so")
ABI_VERSION = 22

AOG_REWARD = {"strehl_ratio": 0, "smf_ssim": 1}
AOG_PRECISION = {"fast": 0, "fp64": 1}
AOG_KERNEL = {"auto": 0, "valu": 1, "mfma": 2}
AOG_SCREENS = {"twoband": 0, "hcipy16": 1}
AOG_EXTRUDE = {"auto": 0, "f64": 1}
AOG_PROF = {"fused": 0, "screen_rows": 1, "screen_cols": 2, "pack": 3, "extrude": 4, "sh_field": 5, "sh_rows_fwd": 6, "sh_cols": 7, "sh_rows_inv": 8}


class AogConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "num_envs", "n_pupil", "n_modes", "obs_dim", "n_ap", "n_wfs_tables", "n_sci_tables",
        "n_fiber_modes", "reward_type", "sh_operation", "max_steps", "flat_mirror_start", "has_rew_threshold",
        "precision", "kernel", "pixel_chunks", "atm_dynamic", "env_id_base", "obs_separable")] + [(n, C.c_double) for n in (
        "wavelength_wfs", "wavelength_sci", "surface_rms_target", "rew_threshold", "ssim_ref_peak", "ssim_alpha")]


class AogTables(C.Structure):
    _fields_ = [("ap_index", C.POINTER(C.c_int32))] + [(n, C.POINTER(C.c_double)) for n in (
        "modes", "gram", "wfs_tables", "sci_tables", "wfs_coef", "sci_coef", "focal_m1", "focal_m2")] + [("n_focal", C.c_int32)]


class AogLayerTables(C.Structure):
    _fields_ = [("nz_vertical", C.c_int32), ("nz_horizontal", C.c_int32),
                ("stencil_vertical", C.POINTER(C.c_int32)), ("stencil_horizontal", C.POINTER(C.c_int32)),
                ("A_vertical", C.POINTER(C.c_double)), ("B_vertical", C.POINTER(C.c_double)),
                ("A_horizontal", C.POINTER(C.c_double)), ("B_horizontal", C.POINTER(C.c_double)),
                ("sqrt_cn_squared", C.c_double), ("pixel_pitch", C.c_double), ("delta_t", C.c_double)]


class AogLayerComposite(C.Structure):
    _fields_ = [("axis", C.c_int32), ("k_max", C.c_int32), ("n_old", C.c_int32), ("reserved0", C.c_int32),
                ("old_yx", C.POINTER(C.c_int32)), ("A", C.POINTER(C.c_double)), ("B", C.POINTER(C.c_double))]


class AogShTables(C.Structure):
    _fields_ = [("n_sub", C.c_int32), ("sub_slot", C.POINTER(C.c_int32))] + [(n, C.POINTER(C.c_double)) for n in (
        "centres", "slopes_ref", "reconstruction", "mla_phase", "transfer", "x_det")] + [(n, C.c_double) for n in (
        "field_amplitude", "image_scale", "gain", "leakage")] + [("fft_double", C.c_int32), ("reserved0", C.c_int32)]


class AogActor(C.Structure):  # mirrors aog_actor in include/aogym.h
    _fields_ = [("batch", C.c_int32), ("state_dim", C.c_int32), ("hidden_dim", C.c_int32), ("act_dim", C.c_int32),
                ("env_id_base", C.c_int32), ("reserved0", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("w3", C.c_void_p), ("b3", C.c_void_p),
                ("wo", C.c_void_p), ("bo", C.c_void_p), ("dropout_p", C.c_float), ("cov_var", C.c_float),
                ("seed", C.c_uint64), ("call_index", C.c_uint64)]


class AogActionNoise(C.Structure):  # mirrors aog_action_noise (action form of a policy query: mode, optional OU state)
    _fields_ = [("mode", C.c_int32), ("reserved0", C.c_int32), ("ou_state", C.c_void_p), ("ou_mu", C.c_double), ("ou_theta", C.c_double),
                ("ou_sigma", C.c_double)]


AOG_ACTION_MODE = {"sample": 0, "mean": 1}


class AogObsMft(C.Structure):  # mirrors aog_obs_mft (ABI 20)
    _fields_ = [("o", C.c_int32), ("reserved0", C.c_int32), ("m1", C.POINTER(C.c_double)), ("m2", C.POINTER(C.c_double))]


class AogPyramidTables(C.Structure):  # mirrors aog_pyramid_tables (additive in ABI 22; natural alignment, no aog_struct_size index)
    _fields_ = [(n, C.c_int32) for n in ("samples", "pixels", "n_mod", "n_valid")] + [(n, C.c_void_p) for n in (
        "m1", "m2", "b1", "b2", "m1s", "m2s", "b1s", "b2s", "valid")] + [(n, C.c_double) for n in ("fwd_unscale", "back_unscale", "photons")]


class AogPredictorConfig(C.Structure):  # mirrors aog_predictor_config (additive in ABI 22; no aog_struct_size index)
    _fields_ = [(n, C.c_int32) for n in ("batch", "act_dim", "order", "env_id_base", "reserved0", "reserved1")] + [(n, C.c_double) for n in (
        "forgetting", "p0", "scale")]


class AogTelemetryConfig(C.Structure):  # mirrors aog_telemetry_config (additive in ABI 22; no aog_struct_size index)
    _fields_ = [(n, C.c_int32) for n in ("batch", "act_dim", "length", "env_id_base")]


class AogSpgdConfig(C.Structure):  # mirrors aog_spgd_config (additive in ABI 22; no aog_struct_size index)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "act_dim", "env_id_base")] + [("seed", C.c_uint64), ("metric", C.c_int32),
                                                                                                  ("reserved0", C.c_int32), ("clip", C.c_double)]


AOG_SPGD_METRIC = {"power": 0, "strehl": 1, "reward": 2}


class AogLinkConfig(C.Structure):  # mirrors aog_link_config (additive in ABI 22; no aog_struct_size index)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "length", "env_id_base", "reserved")]


AOG_LINK_REF = {"absolute": 0, "mean": 1}


class AogDisturbanceConfig(C.Structure):  # mirrors aog_disturbance_config (include/aogym_disturbance.h; its size query is aog_disturbance_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "n_terms", "env_id_base")] + [("seed", C.c_uint64)]


DISTURBANCE_MAX_TERMS = 8   # AOG_DISTURBANCE_MAX_TERMS


class AogServoConfig(C.Structure):  # mirrors aog_servo_config (include/aogym_servo.h; its size query is aog_servo_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "act_dim", "max_latency")]


SERVO_MAX_LATENCY, SERVO_MAX_ACT = 4, 128   # AOG_SERVO_MAX_LATENCY, AOG_SERVO_MAX_ACT


class AogAltMirrorConfig(C.Structure):  # mirrors aog_altmirror_config (include/aogym_conjugate.h; its size query is aog_altmirror_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "n_pixels", "n_modes", "reserved")]


ALTMIRROR_MAX_MODES = 256   # AOG_ALTMIRROR_MAX_MODES


class AogTomoConfig(C.Structure):  # mirrors aog_tomo_config (include/aogym_tomography.h; its size query is aog_tomo_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "n_out", "n_inputs")] + [("width", C.c_int32 * 4), ("env_id_base", C.c_int32),
                                                                                           ("reserved", C.c_int32)]


WAVEFRONT_MAX_SHAPES, TOMO_MAX_OUT, TOMO_MAX_INPUTS, TOMO_MAX_WIDTH = 512, 576, 4, 576   # AOG_WAVEFRONT_MAX_SHAPES, AOG_TOMO_MAX_*


class AogLqgConfig(C.Structure):  # mirrors aog_lqg_config (include/aogym_lqg.h; its size query is aog_lqg_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "act_dim", "n_models", "reserved")]


class AogScintConfig(C.Structure):  # mirrors aog_scint_config (include/aogym_scintillation.h; its size query is aog_scint_config_size)
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "num_envs", "n_pixels", "n_layers", "n_fiber", "reserved")] + [("scratch_bytes", C.c_int64)]


SCINT_MAX_LAYERS, SCINT_MAX_FIBER = 8, 4   # AOG_SCINT_MAX_LAYERS, AOG_SCINT_MAX_FIBER


LQG_MAX_ACT, LQG_MAX_MODELS, LQG_MAX_DELAY, LQG_MAX_ITERATIONS = 128, 4, 4, 4096   # AOG_LQG_MAX_*


class AogInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "num_envs", "num_envs_padded", "n_ap", "n_ap_padded", "n_modes_padded", "pixel_chunks",
        "kernel", "n_sums", "reserved")] + [("device_bytes", C.c_int64)]


# every symbol include/aogym.h declares: name -> (restype, argtypes); the stand-alone handles' lifecycle calls come from STANDALONE below
SYMBOLS = {
    "aog_abi_version": (C.c_int, []),
    "aog_last_error": (C.c_char_p, []),
    "aog_build_id": (C.c_char_p, []),
    "aog_struct_size": (C.c_int64, [C.c_int]),
    "aog_create": (C.c_int, [C.POINTER(AogConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "aog_destroy": (None, [C.c_void_p]),
    "aog_get_info": (C.c_int, [C.c_void_p, C.POINTER(AogInfo)]),
    "aog_upload_tables": (C.c_int, [C.c_void_p, C.POINTER(AogTables)]),
    "aog_upload_obs_mft": (C.c_int, [C.c_void_p, C.POINTER(AogObsMft)]),
    "aog_set_screens_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aog_set_screens_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aog_upload_layer": (C.c_int, [C.c_void_p, C.POINTER(AogLayerTables)]),
    "aog_upload_layer_composite": (C.c_int, [C.c_void_p, C.POINTER(AogLayerComposite)]),
    "aog_set_extrusion_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "aog_set_wind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "aog_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "aog_set_extrusion_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aog_set_rng_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "aog_evolve_atmosphere": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aog_install_layer_sum": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "aog_get_screens_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aog_generate_screens": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "aog_set_turbulence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_set_detector": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_turbulence_factors": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "aog_fused_plan": (C.c_int, [C.c_int] * 7 + [C.c_void_p]),
    "aog_pack_operand_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "aog_reorder_operand_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "aog_set_screen_method": (C.c_int, [C.c_void_p, C.c_int]),
    "aog_upload_sh": (C.c_int, [C.c_void_p, C.POINTER(AogShTables)]),
    "aog_sh_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_sh_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_state_bytes": (C.c_int64, [C.c_void_p]),
    "aog_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "aog_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aog_get_phase_screen": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aog_actor_act": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_actor_act_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AogActionNoise),
                                      C.c_void_p]),
    "aog_reset_act": (C.c_int, [C.c_void_p, C.POINTER(AogActor)] + [C.c_void_p] * 6),
    "aog_reset_act_noise": (C.c_int, [C.c_void_p, C.POINTER(AogActor)] + [C.c_void_p] * 5 + [C.POINTER(AogActionNoise), C.c_void_p]),
    "aog_step_act": (C.c_int, [C.c_void_p, C.POINTER(AogActor)] + [C.c_void_p] * 10 + [C.POINTER(C.c_int), C.c_void_p]),
    "aog_step_act_noise": (C.c_int, [C.c_void_p, C.POINTER(AogActor)] + [C.c_void_p] * 10 + [C.POINTER(C.c_int), C.POINTER(AogActionNoise),
                                                                                            C.c_void_p]),
    "aog_device_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "aog_set_return_accumulator": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aog_get_actuators": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_set_actuators": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_step": (C.c_int, [C.c_void_p] * 9),
    "aog_step_pipelined": (C.c_int, [C.c_void_p] * 10),
    "aog_focal_image": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aog_focal_images": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aog_upload_wavefront_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_wavefront_truth": (C.c_int, [C.c_void_p] * 6),
    "aog_upload_science": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int]),
    "aog_science_integrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_science_clear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_science_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_upload_gradient": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aog_output_gradient": (C.c_int, [C.c_void_p] * 9),
    "aog_upload_gradient_obs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aog_upload_pyramid": (C.c_int, [C.c_void_p, C.POINTER(AogPyramidTables)]),
    "aog_pyramid_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_pyramid_slopes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_upload_pyramid_reconstructor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_pyramid_update": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_pyramid_gradient": (C.c_int, [C.c_void_p] * 9),
    "aog_predictor_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_predictor_update": (C.c_int, [C.c_void_p] * 6),
    "aog_telemetry_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_telemetry_push": (C.c_int, [C.c_void_p] * 4),
    "aog_telemetry_psd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_telemetry_gains": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int] + [C.c_void_p] * 5),
    "aog_spgd_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_spgd_reset": (C.c_int, [C.c_void_p] * 5),
    "aog_spgd_update": (C.c_int, [C.c_void_p] * 5),
    "aog_link_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_link_push": (C.c_int, [C.c_void_p] * 4),
    "aog_link_statistics": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int,
                                      C.POINTER(C.c_double), C.c_int] + [C.c_void_p] * 13),
    "aog_reset_spgd": (C.c_int, [C.c_void_p] * 6),
    "aog_step_spgd": (C.c_int, [C.c_void_p] * 10 + [C.POINTER(C.c_int), C.c_void_p]),
    "aog_selftest_poisson":(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p]),
    "aog_selftest_barrier_timeout": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aog_selftest_sincos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aog_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "aog_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "aog_profile_block": (C.c_int, [C.c_void_p, C.c_int]),
    "aog_profile_read_kernel": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}

# every symbol include/aogym_disturbance.h declares
DISTURBANCE_SYMBOLS = {
    "aog_disturbance_config_size": (C.c_int64, []),
    "aog_disturbance_set_params": (C.c_int, [C.c_void_p] * 7),
    "aog_disturbance_reset": (C.c_int, [C.c_void_p] * 4),
    "aog_disturbance_advance": (C.c_int, [C.c_void_p] * 5),
    "aog_disturbance_coefficients": (C.c_int, [C.c_void_p] * 3),
    "aog_upload_disturbance_basis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aog_install_layer_sum_disturbed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
}

# every symbol include/aogym_sightline.h declares
SIGHTLINE_SYMBOLS = {
    "aog_install_layer_sum_sightline": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}

# every symbol include/aogym_servo.h declares
SERVO_SYMBOLS = {
    "aog_servo_config_size": (C.c_int64, []),
    "aog_servo_set_params": (C.c_int, [C.c_void_p] * 6),
    "aog_servo_reset": (C.c_int, [C.c_void_p] * 3),
    "aog_servo_apply": (C.c_int, [C.c_void_p] * 5),
}

# every symbol include/aogym_conjugate.h declares, the handle's lifecycle calls written out (aog_altmirror is no entry of STANDALONE below)
CONJUGATE_SYMBOLS = {
    "aog_altmirror_config_size": (C.c_int64, []),
    "aog_altmirror_create": (C.c_int, [C.POINTER(AogAltMirrorConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "aog_altmirror_destroy": (None, [C.c_void_p]),
    "aog_altmirror_upload": (C.c_int, [C.c_void_p] * 4),
    "aog_altmirror_set_command": (C.c_int, [C.c_void_p] * 4),
    "aog_altmirror_get": (C.c_int, [C.c_void_p] * 4),
    "aog_altmirror_fit": (C.c_int, [C.c_void_p] * 4),
    "aog_altmirror_state_bytes": (C.c_int64, [C.c_void_p]),
    "aog_altmirror_get_state": (C.c_int, [C.c_void_p] * 3),
    "aog_altmirror_set_state": (C.c_int, [C.c_void_p] * 3),
    "aog_install_layer_sum_conjugate": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p]),
}

# every symbol include/aogym_tomography.h declares, the handle's lifecycle calls written out (aog_tomo is no entry of STANDALONE below)
TOMOGRAPHY_SYMBOLS = {
    "aog_upload_wavefront_shapes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aog_wavefront_project": (C.c_int, [C.c_void_p] * 4),
    "aog_tomo_config_size": (C.c_int64, []),
    "aog_tomo_create": (C.c_int, [C.POINTER(AogTomoConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "aog_tomo_destroy": (None, [C.c_void_p]),
    "aog_tomo_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aog_tomo_update": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_tomo_reset": (C.c_int, [C.c_void_p] * 3),
    "aog_tomo_state_bytes": (C.c_int64, [C.c_void_p]),
    "aog_tomo_get_state": (C.c_int, [C.c_void_p] * 3),
    "aog_tomo_set_state": (C.c_int, [C.c_void_p] * 3),
}

# every symbol include/aogym_shack_gradient.h declares
SHACK_GRADIENT_SYMBOLS = {
    "aog_sh_gradient": (C.c_int, [C.c_void_p] * 9),
}

# every symbol include/aogym_lqg.h declares, the handle's lifecycle calls written out (aog_lqg is no entry of STANDALONE below)
LQG_SYMBOLS = {
    "aog_lqg_config_size": (C.c_int64, []),
    "aog_lqg_create": (C.c_int, [C.POINTER(AogLqgConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "aog_lqg_destroy": (None, [C.c_void_p]),
    "aog_lqg_set_model": (C.c_int, [C.c_void_p] * 6),
    "aog_lqg_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_lqg_update": (C.c_int, [C.c_void_p] * 5),
    "aog_lqg_reset": (C.c_int, [C.c_void_p] * 3),
    "aog_lqg_state_bytes": (C.c_int64, [C.c_void_p]),
    "aog_lqg_get_state": (C.c_int, [C.c_void_p] * 3),
    "aog_lqg_set_state": (C.c_int, [C.c_void_p] * 3),
}

# every symbol include/aogym_cone.h declares
CONE_SYMBOLS = {
    "aog_install_layer_sum_cone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p]),
    "aog_cone_check_geometry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
}

# every symbol include/aogym_scintillation.h declares, the handle's lifecycle calls written out (aog_scint is no entry of STANDALONE below, and has no state)
SCINTILLATION_SYMBOLS = {
    "aog_scint_config_size": (C.c_int64, []),
    "aog_scint_create": (C.c_int, [C.POINTER(AogScintConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "aog_scint_destroy": (None, [C.c_void_p]),
    "aog_scint_upload": (C.c_int, [C.c_void_p] * 3),
    "aog_scint_upload_modes": (C.c_int, [C.c_void_p] * 3),
    "aog_scint_filter": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "aog_scint_correction": (C.c_void_p, [C.c_void_p, C.c_int]),
    "aog_scint_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aog_scint_tile_floats": (C.c_int64, [C.c_void_p]),
    "aog_scint_scratch_bytes": (C.c_int64, [C.c_void_p]),
    "aog_scint_install": (C.c_int, [C.c_void_p] * 6),
    "aog_scint_receive": (C.c_int, [C.c_void_p] * 8),
}


def _lifecycle(prefix, config):
    """The five calls every stand-alone handle has (csrc/standalone_handle.h)."""
    return {prefix + "_create": (C.c_int, [C.POINTER(config), C.c_int, C.POINTER(C.c_void_p)]), prefix + "_destroy": (None, [C.c_void_p]),
            prefix + "_state_bytes": (C.c_int64, [C.c_void_p]), prefix + "_get_state": (C.c_int, [C.c_void_p] * 3),
            prefix + "_set_state": (C.c_int, [C.c_void_p] * 3)}


# the stand-alone handles: prefix -> (config class, the symbols of the header that declares it); their own calls are listed above
STANDALONE = {"aog_predictor": (AogPredictorConfig, SYMBOLS), "aog_telemetry": (AogTelemetryConfig, SYMBOLS), "aog_spgd": (AogSpgdConfig, SYMBOLS),
              "aog_link": (AogLinkConfig, SYMBOLS), "aog_disturbance": (AogDisturbanceConfig, DISTURBANCE_SYMBOLS),
              "aog_servo": (AogServoConfig, SERVO_SYMBOLS)}
for _prefix, (_config, _symbols) in STANDALONE.items():
    _symbols.update(_lifecycle(_prefix, _config))
del _prefix, _config, _symbols

_lib = None


def load():
    """Load (once) and type the shared library.  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or adaptive_optics_gym_amd/build.py) — there is no CPU fallback for the device path.")
    try:  # let torch's bundled ROCm libraries (HIP runtime, hipFFT/rocFFT; same SONAMEs) win if torch is going to be used
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SYMBOLS, **DISTURBANCE_SYMBOLS, **SIGHTLINE_SYMBOLS, **SERVO_SYMBOLS, **CONJUGATE_SYMBOLS, **TOMOGRAPHY_SYMBOLS,
                              **SHACK_GRADIENT_SYMBOLS, **LQG_SYMBOLS, **CONE_SYMBOLS, **SCINTILLATION_SYMBOLS}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.aog_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libaogym.so ABI {lib.aog_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    # the binary must come from the sources beside it (build.py::source_id; developer builds carry "+FLAG" and are accepted on their base id)
    if os.path.isdir(os.path.join(_HERE, "csrc")) and os.environ.get("AOG_SKIP_BUILD_ID_CHECK") != "1":
        from .build import source_id

        have, want = lib.aog_build_id().decode(), source_id()
        if have.split("+")[0] != want:
            raise RuntimeError(f"libaogym.so was built from other sources (build id {have}, sources {want}): run "
                               "`python -m adaptive_optics_gym_amd.build` (or __graft_entry__.build())")
    sized = [(cls, lib.aog_struct_size(which)) for which, cls in enumerate(
        (AogConfig, AogTables, AogLayerTables, AogShTables, AogActor, AogInfo, AogLayerComposite, AogObsMft, AogActionNoise))]
    sized += [(AogDisturbanceConfig, lib.aog_disturbance_config_size()), (AogServoConfig, lib.aog_servo_config_size()),
              (AogAltMirrorConfig, lib.aog_altmirror_config_size()), (AogTomoConfig, lib.aog_tomo_config_size()),
              (AogLqgConfig, lib.aog_lqg_config_size()), (AogScintConfig, lib.aog_scint_config_size())]
    for cls, size in sized:
        if size != C.sizeof(cls):
            raise RuntimeError(f"{cls.__name__}: ctypes layout is {C.sizeof(cls)} bytes, the library's struct {size}")
    _lib = lib
    return lib


class AogError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        msg = load().aog_last_error().decode("utf-8", "replace")
        if "win_size exceeds image extent" in msg:
            raise ValueError(msg)  # what skimage raises in the reference for smf_ssim with obs_dim=2 (AO_env.py:495)
        raise AogError(f"libaogym error {rc}: {msg}")


FUSED_PLAN_FIELDS = ("we", "waves", "heavy", "wg_y", "pair", "chunks_x", "tpc", "n_chunks", "n_ptiles", "n_etiles", "A_pad", "MRW", "lds_tiles",
                     "lds_ring", "valu_qpc", "valu_chunks")


def fused_plan(num_envs, n_ap, n_modes, n_wfs_tables, atm_dynamic=False, pixel_chunks=0, four_wave=False):
    """The fused pupil pass's launch form for a shape, as aog_create would choose it (aog_fused_plan: host arithmetic only, no device)."""
    out = (C.c_int32 * len(FUSED_PLAN_FIELDS))()
    check(load().aog_fused_plan(int(num_envs), int(n_ap), int(n_modes), int(n_wfs_tables), int(bool(atm_dynamic)), int(pixel_chunks),
                                int(bool(four_wave)), out))
    return dict(zip(FUSED_PLAN_FIELDS, out))


TILE_ORDERS = {"natural": 0, "accumulator": 1}   # AOG_TILE_*


def _tile_array(n_blocks, k_pad, out):
    import numpy as np

    shape = (int(n_blocks), int(k_pad) // 16, 4, 64, 8)
    if out is None:
        return np.empty(shape, dtype=np.uint16)
    if out.shape != shape or out.dtype != np.uint16 or not out.flags.c_contiguous:
        raise ValueError(f"operand tiles: out must be a C-contiguous uint16 array of shape {shape}")
    return out


def pack_operand_tiles(m, scale, order, n_blocks, k_pad, out=None):
    """complex m [rows, K] x scale as split-f16 operand tiles [n_blocks, k_pad / 16, 4, 64, 8] uint16 (IEEE half bits) in ``order``
    ('natural' | 'accumulator'), by the library's own packer (aog_pack_operand_tiles: host arithmetic only, no device).  Every element of
    ``out`` (default: a new array) is written."""
    import numpy as np

    m = np.asarray(m, dtype=np.complex128)
    ri = np.ascontiguousarray(np.stack([m.real, m.imag], axis=-1))
    out = _tile_array(n_blocks, k_pad, out)
    check(load().aog_pack_operand_tiles(ri.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], float(scale), TILE_ORDERS[order], int(n_blocks), int(k_pad),
                                        out.ctypes.data_as(C.c_void_p)))
    return out


def reorder_operand_tiles(src, src_order, dst_order, dst_blocks, dst_k_pad, out=None):
    """The tiles of the transposed matrix of the packed table ``src`` [n_blocks, k_pad / 16, 4, 64, 8] uint16, in ``dst_order`` and the
    given shape (aog_reorder_operand_tiles: the halves are copied, nothing is rounded again)."""
    import numpy as np

    src = np.ascontiguousarray(src, dtype=np.uint16)
    out = _tile_array(dst_blocks, dst_k_pad, out)
    check(load().aog_reorder_operand_tiles(src.ctypes.data_as(C.c_void_p), TILE_ORDERS[src_order], src.shape[0], 16 * src.shape[1], TILE_ORDERS[dst_order],
                                           int(dst_blocks), int(dst_k_pad), out.ctypes.data_as(C.c_void_p)))
    return out
