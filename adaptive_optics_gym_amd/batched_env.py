"""``BatchedAOEnv`` — B independent adaptive-optics environments stepped in lock-step on one MI355X.

Host-side mirror of the reference's ``AOEnv`` (``/root/reference/gym_AO/envs/AO_env.py``): same constructor
keywords, same ``reset``/``step`` semantics, but tensors carry a leading env dimension and live on the GPU.
All arithmetic of ``reset``/``step`` runs in ``libaogym.so`` (hand-written HIP, called through the C-ABI of
``include/aogym.h``); PyTorch only owns the buffers and the stream.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .atmosphere_host import (build_layer_tables, cn_squared_from_fried_parameter, integer_shifts, screen_numpy,
                              screens_torch)
from .optics_host import HostTables, build_tables, obs_route_for
from .params import OpticalParams, resolve_detector, resolve_per_env, resolve_turbulence
from .spaces import make_box


def _dptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def _mask_array(mask, num_envs, who):
    """A ``mask`` argument (None: every env; numpy, torch on any device, or a list) as a boolean [num_envs] numpy array; ``who`` names the
    caller in the error."""
    if mask is None:
        return np.ones(num_envs, dtype=bool)
    sel = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask).astype(bool).reshape(-1)
    if sel.size != num_envs:
        raise ValueError(f"{who}: mask must have num_envs entries")
    return sel


class BatchedAOEnv:
    """Constructor keywords = AOEnv's (AO_env.py:17-29) plus:

    num_envs            B
    device              torch device (default ``cuda:0``)
    num_pupil_pixels    pupil grid side N (reference: 240)
    seed                seed of the screen generator (global env g uses seed + g for ``screen_source='numpy'``)
    screen_source       'device' (default: hipFFT synthesis inside libaogym, Philox normals) | 'torch' (same algorithm through
                        torch.fft) | 'numpy' (hcipy's draw order on a numpy legacy stream, float64, host)
    screen_method       'twoband' (default: device synthesis splits the von Karman spectrum into a low band on hcipy's (16 N)^2 grid and a
                        high band on the (2 N)^2 grid — the same stationary Gaussian field on the pupil to < 1e-4 of its variance at every
                        lag, 60x fewer spectrum samples) | 'hcipy16' (the literal (16 N)^2 draw); only ``screen_source='device'`` reads it
    screens             optional [B, N, N] achromatic screens to use instead of generating them
    global_env_offset   global id of env 0 of this instance (multi-GPU: ``sharding.shard_range(total, rank, world)[0]``)
    total_envs          size of the global batch this instance is a contiguous slice of (default: offset + num_envs).
                        Every per-env random stream (wind direction, device screen synthesis, extrusion normals, photon noise,
                        numpy per-env seeds) is keyed by the GLOBAL env id, so a batch split over several instances / GPUs
                        gives bit-identical screens to one instance holding all of it
    sh_fft_precision    'single' (default: complex64 Fresnel transforms in the Shack-Hartmann chain; error ~1e-6 of the image peak, far
                        below the photon noise added before the image is read) | 'double' (complex128, for comparing the noise-free
                        sensor image with a float64 oracle)
    precision           'fast' (fp32 data, float64 accumulators) | 'fp64' (validation kernel)
                        obs_dim 1 .. 32 on both.  The observation takes the table route where it is built (fast obs_dim <= 5, fp64
                        obs_dim <= 7) and the separable matrix Fourier transform above (``optics_host.obs_route_for``)
    extrusion           'auto' (dynamic atmosphere: the int8 matrix-core composite form, new samples good to ~1e-9 rad) | 'f64' (float64 round
                        kernels only: the validation form, bit-comparable with the oracle's recursion to 1e-12)
    kernel              'auto' | 'mfma' | 'valu'

    ``atm_fried`` and ``atm_vel`` take a scalar (every env, as the reference) or one value per env: ``num_envs`` values, or ``total_envs``
    values indexed by global env id (sliced at ``global_env_offset``: the slices of a split batch see the values of the unsplit one).
    Speeds are coerced per entry like the reference's scalar (AO_env.py:200-208).  ``fried_parameters`` / ``wind_speeds`` [B] float64
    hold what each env runs at; ``Cn_squared`` is a scalar when every env has the same value, else [B].  Env e of a mixed batch draws
    and evolves exactly what a uniform instance at (r0_e, v_e) would (dynamic int8 extrusion: bit for bit for the envs at the batch's
    largest Cn^2, the tables' value; to ~1e-9 rad per new sample for the others, like the int8 form against the float64 one).
    ``set_turbulence`` changes r0 per episode (domain randomisation); per-env speed is fixed at construction (it sets k_max).

    ``obs_photons`` (default None: the exact focal-plane powers, as the reference) switches the photodetector model on: expected
    photo-electrons per frame of the whole unit-power beam, with ``obs_read_noise`` (electrons rms per pixel and frame) and
    ``obs_background`` (electrons per pixel and frame, subtracted again); each a scalar, ``num_envs`` or ``total_envs`` values like
    ``atm_fried``.  Pixel j of env e then reads (Poisson(F_e c_j + b_e) + sigma_e g_j - b_e) / F_e around its clean value c_j
    (``aog_set_detector``).  Only the observation is noisy: reward, power, Strehl, done, screens and mirror are those of the same env without
    a detector, bit for bit — the reward is the training signal of the true state.  The noise is drawn inside the step kernels from a
    Philox stream keyed by (seed, global env id, pixel, frame), so split batches reproduce whole ones and ``get_state`` / ``set_state``
    resume it.  ``set_detector`` changes the values per episode; ``detector_parameters`` shows them.

    ``science_window`` (default None: no camera) switches the science camera on: an even number w of focal samples, 2 .. 240; the camera
    sees the centred w x w window of the science arm's 240 x 240 focal grid (4 samples per lambda_sci / D) and keeps one float64 long
    exposure per env.  ``science_integrate`` adds the current frame (normalised so that its centre pixel is that step's Strehl ratio),
    ``science_clear`` empties, ``science_exposure`` reads the mean PSF, its Strehl and the encircled energy inside ``science_radii``
    (lambda_sci / D; default 1, 2, 3, 5, 8 clipped to the window).  Off the step path: a step computes the same bits with or without it.

    ``pyramid`` (default None: no sensor) switches the modulated pyramid wavefront sensor on: ``dict(samples=w_q, q=2, pixels=n_s, n_mod=8,
    r_mod=3.0, photons=None, poke=0.01 lambda_wfs, rcond=1e-3, gain=0.4)`` — w_q focal samples per quadrant side at q per lambda_wfs / D, an
    n_s x n_s image per quadrant, n_mod points on a circle of r_mod lambda / D (``pyramid_host``; ValueError for sizes it is not built for).
    ``pyramid_frames`` / ``pyramid_slopes`` read the sensor at the state the last reset or step left, ``PYR_step`` runs its integrator
    (``pyramid_calibrate``, lazily: push-pull pokes of ``poke`` metres through the device sensor on a flat scratch env, Tikhonov inverse with
    ``rcond``); ``photons`` adds photon noise from a Philox stream keyed by (seed, global env id, pixel, sensor call).  Off the step path.  The response
    is linear in small tilts only when the modulation points sit closer than a spot width, 2 pi r_mod / n_mod <~ 1 lambda / D: the default 8
    points at r_mod = 3 close the loop (the integrator converges) but respond quadratically below 1 lambda / D; take n_mod = 32 at r_mod = 3,
    or 12 at 1.5, for a linear sensor (``profiles/pyramid_wfs.md``).

    ``obs_gradient`` (default False) switches the observation gradient of the separable observation route on (``obs_dim`` 6 .. 32; float64
    envs from 8): ``output_gradient`` then takes ``g_obs`` and returns the float64 ``obs_raw`` in its values, and ``autograd.step_outputs``
    differentiates through the observation.  ``ValueError`` on a table-route env, which has that gradient already; ``env.obs_gradient``
    reads the flag.  Off the step path as well; its work buffers are allocated by the first ``output_gradient`` call.

    ``servo`` (default None: ``step(a)`` sets the mirror to ``a`` at once and exactly, and the env launches what it always launched) puts a
    mirror servo between the action and the mirror: ``dict(latency=0.0, response=1.0, stroke=None, stuck=None, max_latency=None)`` — frames of
    loop latency (fractional allowed), the mirror's first-order response, its drive range and its dead actuators, each as
    ``servo.MirrorServo`` takes them — or a ``MirrorServo`` made for this env (the env closes it).  ``env.servo`` is the object.  ``step``
    steps with ``servo.apply(actions)`` and returns it as ``info["applied_action"]``; ``reset(mask)`` puts the selected envs' servo to rest
    when ``flat_mirror_start_per_episode`` is true (the mirror is flat then, and so is its history) and leaves it alone otherwise;
    ``get_state`` / ``set_state`` carry its state under ``"servo"``; ``set_actuators`` bypasses it and leaves it untouched.  The forms that
    make or load the action inside a launch — ``step(next_actions=...)``, ``step_with_policy`` / ``reset_with_policy``, ``step_with_spgd`` /
    ``reset_with_spgd`` — raise ``RuntimeError`` on such an env; ``rollout`` runs its unfused loop.  A controller's loop delay is then
    ``1 + latency`` frames (``telemetry.gain_limit``, ``ModalIntegrator(delay=...)``).
    """

    def __init__(self, num_envs=1, device=None, atm_type="quasi_static", atm_vel=0, atm_fried=0.15,
                 act_type="num_actuators", act_dim=64, obs_dim=2, rew_type="strehl_ratio", rew_threshold=None,
                 timesteps_per_episode=20, flat_mirror_start_per_episode=True, SH_operation=False, *,
                 num_pupil_pixels=240, seed=None, screen_source="device", screen_oversampling=16, screens=None,
                 precision="fast", kernel="auto", pixel_chunks=0, rng=None, verbose=True, params=None,
                 global_env_offset=0, total_envs=None, sh_fft_precision="single", screen_method="twoband", tables=None, extrusion="auto",
                 obs_photons=None, obs_read_noise=0.0, obs_background=0.0, science_window=None, science_radii=None, obs_gradient=False, pyramid=None,
                 servo=None):
        import torch

        self._handle = None   # (first: close() and accumulate_returns() read it on an env whose construction failed below)
        self.servo = None
        self._returns_ref = None
        self._torch = torch
        self.lib = _lib.load()  # raises if the HIP extension is missing — no CPU fallback
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedAOEnv needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise RuntimeError("BatchedAOEnv runs on a HIP device only")
        if rew_type not in _lib.AOG_REWARD:
            # the reference leaves `reward` undefined in this case (AO_env.py:476,487); raise something clear instead
            raise ValueError("rew_type must be 'strehl_ratio' or 'smf_ssim'")
        if atm_type not in ("quasi_static", "semi_dynamic", "dynamic"):
            raise ValueError("atm_type must be 'quasi_static', 'semi_dynamic' or 'dynamic'")

        self.num_envs = int(num_envs)
        self.global_env_offset = int(global_env_offset)
        self.total_envs = int(total_envs) if total_envs is not None else self.global_env_offset + self.num_envs
        if self.global_env_offset < 0 or self.global_env_offset + self.num_envs > self.total_envs:
            raise ValueError("global_env_offset / total_envs: this instance's envs must lie inside range(total_envs)")
        self.atm_type = atm_type
        self.rew_type = rew_type
        self.act_type = act_type
        self.flat_mirror_start_per_episode = bool(flat_mirror_start_per_episode)
        self.rew_threshold = rew_threshold
        self.SH_operation = bool(SH_operation)
        if sh_fft_precision not in ("single", "double"):
            raise ValueError("sh_fft_precision must be 'single' or 'double'")
        self.sh_fft_precision = sh_fft_precision
        turb = resolve_turbulence(atm_type, atm_fried, atm_vel, self.num_envs, self.total_envs, self.global_env_offset, verbose)
        self._detector = resolve_detector(obs_photons, obs_read_noise, obs_background, self.num_envs, self.total_envs, self.global_env_offset)
        self._last_obs = self.last_obs_raw = None
        self.observation_frames = 0   # observations written so far (every reset / step adds one): the frame of the detector's random stream
        fried, self._fried_all, vel_scalar = turb["fried"], turb["fried_all"], turb["vel_scalar"]
        self.velocity, self._wind_speeds = turb["velocity"], turb["speeds"]
        self.fried_parameter = atm_fried if turb["fried_scalar"] else fried.copy()
        self._fried = fried
        self.params = params if params is not None else OpticalParams(num_pupil_pixels=int(num_pupil_pixels))
        self.num_pupil_pixels = self.params.num_pupil_pixels
        self.num_modes = int(act_dim)
        self.obs_dim = int(obs_dim)
        self.num_focal_pixels_fiber_subsample = int(obs_dim)
        self.max_steps = timesteps_per_episode
        self.delta_t = self.params.delta_t
        self.wavelength_wfs = self.params.wavelength_wfs
        self.wavelength_sci = self.params.wavelength_sci
        self.timestep = 0
        self.episode_no = 0
        self.seed = seed
        self.screen_source = screen_source
        self.screen_oversampling = int(screen_oversampling)
        if screen_method not in _lib.AOG_SCREENS:
            raise ValueError("screen_method must be 'twoband' or 'hcipy16'")
        self.screen_method = screen_method
        if extrusion not in _lib.AOG_EXTRUDE:
            raise ValueError("extrusion must be 'auto' or 'f64'")
        self._extrusion = extrusion
        self._rng = rng
        self._rngs = {}                # screen_source='numpy' with a seed: env -> its RandomState (_env_rng)
        self._gen = None               # screen_source='torch': the instance's torch.Generator (_generate_screens)
        self._host_rng = self._rng is not None or screen_source == "numpy"
        self._lib_seeded = False       # see _seed_library()
        self._lib_per_env = False      # the library holds per-env Cn^2 (_push_turbulence)
        self._lib_detector = False     # the library holds detector values (_push_detector)
        # host arrays / device tensors a library call reads: kept alive here
        self._cn2_keep = self._layer = self._noise_dev = self._next_actions_keepalive = None
        self._trunc = None
        self._persistent_out = False   # see persistent_outputs()
        self._step_cache = None        # (views of the persistent block + their addresses)
        self._pack = None
        self._wavefront_fit_uploaded = False
        self._science = None           # optics_host.ScienceTables of the science camera (science_window)
        self._science_uploaded = False
        self.science_window = self.science_radii = None
        self.pyramid = None            # the sensor's settings (pyramid=dict(...)), its host tables and what was uploaded
        self._pyramid = None
        self._pyramid_uploaded = False
        self._pyramid_calibrated = False
        self.pyramid_frame_count = 0   # sensor calls since the upload: the frame of the photon stream
        self._precision, self._kernel, self._pixel_chunks = precision, kernel, pixel_chunks

        self.observation_space = make_box(-1, 1, (self.obs_dim ** 2,), np.float16)  # AO_env.py:45
        self.action_space = make_box(-1, 1, (self.num_modes,), np.float16)          # AO_env.py:46

        self._set_cn2(fried)
        # the int8 extrusion's tables carry the largest Cn^2 of the WHOLE batch the values were given for (so that split == whole)
        self._cn2_table = max(cn_squared_from_fried_parameter(float(r), self.params.wavelength_sci) for r in self._fried_all)
        if precision not in _lib.AOG_PRECISION:
            raise ValueError("precision must be 'fast' or 'fp64'")
        self.obs_route = obs_route_for(precision, self.obs_dim)
        if obs_gradient and self.obs_route != "separable":
            raise ValueError("obs_gradient=True switches the observation gradient of the separable observation route on; this env takes the table "
                             "route, where output_gradient has it already")
        self._obs_gradient = bool(obs_gradient)
        # (tables=: the HostTables of another instance with the same params / act_type / act_dim / obs_dim / route, to skip the host precompute)
        if tables is not None and tables.obs_route != self.obs_route:
            raise ValueError(f"tables= were built for the {tables.obs_route!r} observation route; this handle takes {self.obs_route!r}")
        self.tables: HostTables = tables if tables is not None else build_tables(self.params, act_type, self.num_modes, self.obs_dim,
                                                                                 obs_route=self.obs_route)
        if science_window is not None:
            from .optics_host import science_tables

            self._science = science_tables(self.params, science_window, science_radii)   # (ValueError before anything is created)
            self.science_window = self._science.window
            self.science_radii = self._science.radii.copy()
        elif science_radii is not None:
            raise ValueError("science_radii without science_window: the science camera is off")
        if pyramid is not None:
            from .pyramid_host import pyramid_tables

            cfg = dict(samples=32, q=2, pixels=32, n_mod=8, r_mod=3.0, photons=None, poke=0.01 * self.params.wavelength_wfs, rcond=1e-3, gain=0.4)
            unknown = set(pyramid) - set(cfg)
            if unknown:
                raise ValueError(f"pyramid: unknown keys {sorted(unknown)}")
            cfg.update(pyramid)
            if cfg["photons"] is not None and not (np.isfinite(cfg["photons"]) and cfg["photons"] > 0):
                raise ValueError("pyramid: photons must be None or a positive number")
            if not (cfg["poke"] > 0 and cfg["rcond"] > 0 and np.isfinite(cfg["gain"])):
                raise ValueError("pyramid: poke and rcond must be positive, gain finite")
            self._pyramid = pyramid_tables(self.num_pupil_pixels, self.tables.n_ap, cfg["samples"], cfg["q"], cfg["pixels"], cfg["n_mod"],
                                           cfg["r_mod"])   # (ValueError before anything is created)
            self.pyramid = cfg
        servo_plan = self._servo_plan(servo)   # (ValueError before anything is created)
        self._create_handle(precision, kernel, pixel_chunks)
        self._upload_tables()
        layer = self._draw_wind_and_stencils()
        theta = self.wind_u * 2 * np.pi
        speed = float(self.velocity) if vel_scalar else self._wind_speeds[:, None]
        self.velocity_vectors = speed * np.stack([np.cos(theta), np.sin(theta)], axis=1)  # [B, 2] m/s
        if self.atm_type == "dynamic":
            self._upload_layer(layer)
        self._push_turbulence()
        if screens is not None:
            self.set_screens(screens)
        else:
            self._generate_screens()
        if self.SH_operation:
            self._upload_shack_hartmann()
        self._push_detector()   # (last: in host-RNG mode without a seed it draws the handle's seed after the reference's own draws)
        if servo_plan is not None:
            from .servo import MirrorServo

            self.servo = servo if isinstance(servo, MirrorServo) else MirrorServo(self, **servo_plan)

    def _servo_plan(self, servo):
        """``servo=``: None, a dict of ``MirrorServo``'s keywords (checked here; returned for the constructor) or a ``MirrorServo`` made for
        this env's batch, action width, global env ids and device."""
        if servo is None:
            return None
        from .servo import MirrorServo, resolve_servo

        if isinstance(servo, MirrorServo):
            index = self.device.index if self.device.index is not None else self._torch.cuda.current_device()
            mine = (self.num_envs, self.num_modes, self.global_env_offset, index)
            if (servo.num_envs, servo.act_dim, servo.global_env_offset, servo.device.index) != mine:
                raise ValueError(f"servo: made for {servo.num_envs} envs x {servo.act_dim} actuators from global id {servo.global_env_offset} on "
                                 f"{servo.device}, this env has {self.num_envs} x {self.num_modes} from {self.global_env_offset} on {self.device}")
            return {}
        if not isinstance(servo, dict) or not set(servo) <= {"latency", "response", "stroke", "stuck", "max_latency"}:
            raise ValueError("servo: a dict with any of 'latency', 'response', 'stroke', 'stuck' and 'max_latency', or a MirrorServo")
        resolve_servo(self.num_envs, self.total_envs, self.global_env_offset, self.num_modes, **servo)
        return dict(servo)

    def _refuse_with_servo(self, who, instead, why=None):
        if self.servo is not None:
            why = why or f"{who} forms or loads the action inside a launch, where the servo has no place"
            raise RuntimeError(f"{who}: this env has a mirror servo attached; {why} — use {instead}")

    def _create_handle(self, precision, kernel, pixel_chunks):
        """Fill the library's aog_config from this instance, create the handle on the env's device and give it its seed."""
        t = self.tables
        cfg = _lib.AogConfig()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.num_envs = self.num_envs
        cfg.n_pupil = self.num_pupil_pixels
        cfg.n_modes = self.num_modes
        cfg.obs_dim = self.obs_dim
        cfg.n_ap = t.n_ap
        cfg.n_wfs_tables = t.wfs_tables.shape[0]
        cfg.n_sci_tables = t.sci_tables.shape[0]
        cfg.n_fiber_modes = t.n_fiber_modes
        cfg.reward_type = _lib.AOG_REWARD[self.rew_type]
        cfg.sh_operation = int(self.SH_operation)
        cfg.max_steps = int(self.max_steps)
        cfg.flat_mirror_start = int(self.flat_mirror_start_per_episode)
        cfg.has_rew_threshold = int(self.rew_threshold is not None)
        cfg.precision = _lib.AOG_PRECISION[precision]
        cfg.kernel = _lib.AOG_KERNEL[kernel]
        cfg.pixel_chunks = int(pixel_chunks)
        cfg.atm_dynamic = int(self.atm_type == "dynamic")
        cfg.env_id_base = self.global_env_offset
        cfg.obs_separable = int(self.obs_route == "separable")
        cfg.wavelength_wfs = self.params.wavelength_wfs
        cfg.wavelength_sci = self.params.wavelength_sci
        cfg.surface_rms_target = self.params.action_rms_fraction * self.params.wavelength_sci
        cfg.rew_threshold = float(self.rew_threshold) if self.rew_threshold is not None else 0.0
        cfg.ssim_ref_peak = self.params.ssim_ref_peak
        cfg.ssim_alpha = self.params.ssim_alpha
        self._handle = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else self._torch.cuda.current_device()
        _lib.check(self.lib.aog_create(C.byref(cfg), dev_index, C.byref(self._handle)))
        self._seed_library(draw=False)

    def _upload_tables(self):
        """The host tables (and, separable route, the observation's transform matrices) to the handle; then its screen method and ``info``."""
        t = self.tables
        keep = dict(
            ap=np.ascontiguousarray(t.ap_index, dtype=np.int32),
            modes=np.ascontiguousarray(t.modes, dtype=np.float64),
            gram=np.ascontiguousarray(t.gram, dtype=np.float64),
            wt=np.ascontiguousarray(t.wfs_tables, dtype=np.float64),
            st=np.ascontiguousarray(t.sci_tables, dtype=np.float64),
            wc=np.ascontiguousarray(np.stack([t.wfs_coef.real, t.wfs_coef.imag], axis=-1), dtype=np.float64),
            sc=np.ascontiguousarray(np.stack([t.sci_coef.real, t.sci_coef.imag], axis=-1), dtype=np.float64),
            m1=np.ascontiguousarray(np.stack([t.focal_m1.real, t.focal_m1.imag], axis=-1), dtype=np.float64),
            m2=np.ascontiguousarray(np.stack([t.focal_m2.real, t.focal_m2.imag], axis=-1), dtype=np.float64),
        )
        tabs = _lib.AogTables(_dptr(keep["ap"], C.c_int32), _dptr(keep["modes"], C.c_double), _dptr(keep["gram"], C.c_double),
                              _dptr(keep["wt"], C.c_double), _dptr(keep["st"], C.c_double), _dptr(keep["wc"], C.c_double),
                              _dptr(keep["sc"], C.c_double), _dptr(keep["m1"], C.c_double), _dptr(keep["m2"], C.c_double),
                              int(t.focal_m1.shape[0]))
        _lib.check(self.lib.aog_upload_tables(self._handle, C.byref(tabs)))
        self._wavefront_fit_uploaded = False   # (the library drops the wavefront fit with the old tables; wavefront_truth uploads it again)
        self._science_uploaded = False         # (and the science camera)
        self._gradient_uploaded = False        # (and the gradient's operand tables, the observation's among them; output_gradient uploads them again)
        self._upload_keep = (keep, tabs)       # (output_gradient hands the same host tables to aog_upload_gradient)
        self._upload_science()
        self._pyramid_uploaded = self._pyramid_calibrated = False   # (and the pyramid sensor, with its reconstructor)
        self._upload_pyramid()
        if self.obs_route == "separable":
            om1 = np.ascontiguousarray(np.stack([t.obs_m1.real, t.obs_m1.imag], axis=-1), dtype=np.float64)
            om2 = np.ascontiguousarray(np.stack([t.obs_m2.real, t.obs_m2.imag], axis=-1), dtype=np.float64)
            mft = _lib.AogObsMft(self.obs_dim, 0, _dptr(om1, C.c_double), _dptr(om2, C.c_double))
            _lib.check(self.lib.aog_upload_obs_mft(self._handle, C.byref(mft)))
            self._obs_mft_keep = (om1, om2, mft)   # (output_gradient hands the same host matrices to aog_upload_gradient_obs)
        _lib.check(self.lib.aog_set_screen_method(self._handle, _lib.AOG_SCREENS[self.screen_method]))
        self.info = _lib.AogInfo()
        _lib.check(self.lib.aog_get_info(self._handle, C.byref(self.info)))

    def _draw_wind_and_stencils(self):
        """atmosphere (AO_env.py:361-370): set ``wind_u`` (every env's wind direction / 2 pi) and return the dynamic atmosphere's layer
        tables (None otherwise)."""
        # hcipy's construction order: wind direction (rand), the two stencil draws (geometric x2), then
        # the screen normals.  Host-RNG mode consumes the numpy stream in that order; env 0's draws define the stencils /
        # AR matrices shared by the whole batch (for B = 1 this is exactly the reference's layer).
        N = self.num_pupil_pixels
        wind_u = np.zeros(self.num_envs)   # hcipy draws theta = rand() * 2 pi per layer
        layer = None
        # GLOBAL env 0's draws define the stencils whatever slice of the batch this instance holds.
        if self._host_rng:
            if self.atm_type == "dynamic" and self.global_env_offset > 0 and self._rng is None and self.seed is not None:
                r0 = np.random.RandomState(self.seed)      # global env 0's stream, replayed: rand() then the two stencil draws
                r0.rand()
                layer = build_layer_tables(N, self.params.pupil_pixel, self.params.outer_scale, r0)
            for e in range(self.num_envs):
                r = self._env_rng(e)
                wind_u[e] = r.rand()
                if e == 0 and self.atm_type == "dynamic" and layer is None:
                    layer = build_layer_tables(N, self.params.pupil_pixel, self.params.outer_scale, r)
                else:
                    r.geometric(0.5, N)
                    r.geometric(0.5, N)
        else:
            base_seed = self._base_seed
            trng = np.random.RandomState(base_seed)
            wind_u = trng.rand(self.total_envs)[self.global_env_offset:self.global_env_offset + self.num_envs]
            if self.atm_type == "dynamic":
                # the stencil draws have a stream of their own: drawn after the wind directions they would depend on total_envs,
                # and instances holding different slices of one batch must share the AR matrices whatever total_envs they were given
                layer = build_layer_tables(N, self.params.pupil_pixel, self.params.outer_scale, np.random.RandomState([base_seed & 0xFFFFFFFF, 0x57E9C11]))
        self.wind_u = np.array(wind_u, dtype=np.float64)
        return layer

    # ------------------------------------------------------------------------------------------------
    # per-env turbulence
    @property
    def fried_parameters(self):
        """[B] float64 Fried parameter of every env (read-only view)."""
        v = self._fried.view()
        v.flags.writeable = False
        return v

    @property
    def wind_speeds(self):
        """[B] float64 wind speed of every env after the reference's coercion (read-only view)."""
        v = self._wind_speeds.view()
        v.flags.writeable = False
        return v

    def _set_cn2(self, fried):
        wl = self.params.wavelength_sci
        self._cn2 = np.array([cn_squared_from_fried_parameter(float(r), wl) for r in fried], dtype=np.float64)
        uniform = self.num_envs > 0 and bool(np.all(self._cn2 == self._cn2[0]))
        self.Cn_squared = float(self._cn2[0]) if uniform else self._cn2.copy()

    def _per_env_turbulence(self):
        """True when the library needs per-env values: the envs differ, or (dynamic) they differ from the int8 tables' Cn^2."""
        if isinstance(self.Cn_squared, np.ndarray):
            return True
        return self.atm_type == "dynamic" and self.Cn_squared != self._cn2_table

    def _screen_cn2(self):
        """The cn_squared argument of aog_generate_screens: the handle-wide value, or (per-env values set) one it only validates."""
        return float(self._cn2_table) if self._per_env_turbulence() else float(self.Cn_squared)

    def _push_turbulence(self):
        """Hand the per-env Cn^2 to the library (aog_set_turbulence), or NULL when every env runs at the handle-wide value."""
        if self._per_env_turbulence():
            self._cn2_keep = np.ascontiguousarray(self._cn2, dtype=np.float64)
            _lib.check(self.lib.aog_set_turbulence(self._handle, self._cn2_keep.ctypes.data_as(C.c_void_p), self._stream()))
            self._lib_per_env = True
        elif self._lib_per_env:
            _lib.check(self.lib.aog_set_turbulence(self._handle, None, self._stream()))
            self._lib_per_env = False

    def set_turbulence(self, fried, mask=None):
        """New Fried parameters for the envs selected by ``mask`` (default all): per-episode domain randomisation of r0.  ``fried``: a
        scalar, ``num_envs`` or ``total_envs`` values (as ``atm_fried``); only the masked envs' entries are used.

        When it takes effect: ``semi_dynamic`` at those envs' next ``reset`` (the reference redraws the screen there, AO_env.py:76-77);
        ``quasi_static`` and ``dynamic`` redraw the masked envs' screens NOW, on the path a masked semi_dynamic reset takes (device / numpy
        / torch screen source alike).  Dynamic atmosphere: the extrusion of the masked envs follows the new values from the next step on.
        Its tables carry the largest Cn^2 (smallest r0) the constructor was given — over the whole ``total_envs`` batch when that many
        values were passed — and each env's normals are scaled by sqrt(Cn^2_e / Cn^2_table) <= 1, so an r0 below that smallest one raises
        ``ValueError`` (the library refuses it too): build the env with the smallest r0 the randomisation will draw among its ``atm_fried``.
        Per-env wind speed stays what the constructor was given."""
        fried, _, _ = resolve_per_env("fried", fried, self.num_envs, self.total_envs, self.global_env_offset)
        if np.any(fried <= 0):
            raise ValueError("set_turbulence: Fried parameters must be > 0")
        sel = _mask_array(mask, self.num_envs, "set_turbulence")
        new = self._fried.copy()
        new[sel] = fried[sel]
        self._apply_fried(new)
        if self.atm_type != "semi_dynamic" and sel.any():
            self._generate_screens(mask=None if sel.all() else sel)

    def _apply_fried(self, new):
        new = np.asarray(new, dtype=np.float64).copy()
        if self.atm_type == "dynamic":
            wl = self.params.wavelength_sci
            top = max(cn_squared_from_fried_parameter(float(r), wl) for r in new)
            if top > self._cn2_table:
                r_min = float((self._cn2_table * 0.423 * (2 * np.pi / wl) ** 2) ** (-3.0 / 5.0))
                raise ValueError(f"set_turbulence: r0 = {float(new.min()):.4g} m is below the smallest r0 ({r_min:.4g} m) the dynamic atmosphere's "
                                 "extrusion tables were made for; build the env with that r0 among its atm_fried values")
        self._fried = new
        self.fried_parameter = float(self._fried[0]) if bool(np.all(self._fried == self._fried[0])) else self._fried.copy()
        self._set_cn2(self._fried)
        self._push_turbulence()

    # ------------------------------------------------------------------------------------------------
    # photodetector model of the observations
    @property
    def detector_parameters(self):
        """None without a detector, else {"photons", "read_noise", "background"}: [B] float64 read-only views of what each env runs at."""
        if self._detector is None:
            return None
        out = {}
        for k, a in self._detector.items():
            v = a.view()
            v.flags.writeable = False
            out[k] = v
        return out

    @property
    def _base_seed(self):
        """The number the instance's seeded streams start from: ``seed``, or 1234 when it is None."""
        return 1234 if self.seed is None else int(self.seed)

    def _seed_library(self, draw, provisional=False):
        """The handle's 64-bit rng_seed, set once.  Device random streams: ``seed`` (1234 when None), whatever else the constructor does
        (screens= on a static atmosphere seeds no stream otherwise).  Host-RNG mode with a ``seed`` and no ``rng``: that seed too (the
        same on every slice of a split batch).  Otherwise (``rng=`` or the process-global numpy stream: the single-env wrapper) there is
        no number to take, so — only when a detector needs one (``draw``) — 62 bits are drawn from that stream: two instances then
        draw different detector noise, and seeding the stream reproduces it.  Envs without a detector never consume host draws here.
        ``provisional`` (``_upload_layer``): that last case on a dynamic atmosphere meanwhile runs at the base seed, which the handle's
        state blob records and ``sh_update(None)`` draws from; a detector's draw still replaces it."""
        if self._lib_seeded:
            return
        final = True
        if not self._host_rng or (self._rng is None and self.seed is not None):
            value = self._base_seed
        elif draw:
            r = self._env_rng(0)
            value = (int(r.randint(0, 2 ** 31)) << 31) | int(r.randint(0, 2 ** 31))
        elif provisional:
            value, final = self._base_seed, False
        else:
            return
        _lib.check(self.lib.aog_set_rng_seed(self._handle, C.c_uint64(value)))
        self._lib_seeded = final

    def _push_detector(self):
        """Hand the per-env detector values to the library (aog_set_detector), or NULL without a detector."""
        d = self._detector
        if d is None:
            if self._lib_detector:
                _lib.check(self.lib.aog_set_detector(self._handle, None, None, None, self._stream()))
            self._lib_detector = False
            return
        self._seed_library(draw=True)
        ptr = [d[k].ctypes.data_as(C.c_void_p) for k in ("photons", "read_noise", "background")]
        _lib.check(self.lib.aog_set_detector(self._handle, *ptr, self._stream()))   # (the library copies the values before it returns)
        self._lib_detector = True

    def set_detector(self, photons, read_noise=None, background=None, mask=None):
        """New detector values for the envs selected by ``mask`` (default all), from the next observation on: per-episode randomisation
        of the light level.  Each argument as ``obs_photons`` / ``obs_read_noise`` / ``obs_background``; ``read_noise`` / ``background`` =
        None keep the current values (0 when there was no detector).  ``photons=None`` switches the detector off for every env (``mask``
        must be None then): the env is again the noise-free one, bit for bit."""
        if photons is None:
            if mask is not None:
                raise ValueError("set_detector(None) switches the detector off for the whole batch; mask must be None")
            self._detector = None
            self._push_detector()
            return
        cur = self._detector
        new = resolve_detector(photons, 0.0 if read_noise is None else read_noise, 0.0 if background is None else background,
                               self.num_envs, self.total_envs, self.global_env_offset)
        if cur is not None:
            if read_noise is None:
                new["read_noise"] = cur["read_noise"].copy()
            if background is None:
                new["background"] = cur["background"].copy()
        sel = _mask_array(mask, self.num_envs, "set_detector")
        if cur is None and not sel.all():
            raise ValueError("set_detector: the env has no detector yet; the first call must cover every env")
        if cur is not None and not sel.all():
            new = {k: np.where(sel, v, cur[k]) for k, v in new.items()}
        self._detector = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in new.items()}
        self._push_detector()

    def _obs_buffers(self, masked):
        """Fresh (obs float16, obs_raw float32) [B, o^2] for a reset.  A masked reset may write the masked envs' rows only (an env with a
        detector draws for them alone; a handle that keeps its reset observation copies them alone) and leaves the other rows as they are:
        those start as copies of the last observation."""
        torch = self._torch
        n = self.obs_dim ** 2
        if masked and self._last_obs is not None:
            return self._last_obs.clone(), self.last_obs_raw.clone()
        new = torch.zeros if masked and self._detector is not None else torch.empty
        return (new((self.num_envs, n), dtype=torch.float16, device=self.device), new((self.num_envs, n), dtype=torch.float32, device=self.device))

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _env_rng(self, e):
        if self._rng is not None:
            return self._rng
        if self.seed is None:
            return np.random
        if e not in self._rngs:
            self._rngs[e] = np.random.RandomState(self.seed + self.global_env_offset + e)   # seed + GLOBAL env id
        return self._rngs[e]

    def _generate_screens(self, mask=None):
        """New screens from ``screen_source`` for every env, or for those ``mask`` selects."""
        torch = self._torch
        p = self.params
        sel = _mask_array(mask, self.num_envs, "reset")   # (set_turbulence has checked its own)
        if self._host_rng:
            for e in np.flatnonzero(sel):
                psi = screen_numpy(p.num_pupil_pixels, p.pupil_pixel, float(self._cn2[e]), p.outer_scale, self._env_rng(int(e)),
                                   self.screen_oversampling)
                self.set_screens(psi[None], first=int(e))
        elif self.screen_source == "device":
            args = (int(self.screen_oversampling), self._screen_cn2(), float(p.outer_scale), float(p.pupil_pixel), self._stream())
            idx = np.flatnonzero(sel)   # one call per run of consecutive envs (no mask: the whole batch)
            for r in np.split(idx, np.flatnonzero(np.diff(idx) != 1) + 1) if idx.size else []:
                _lib.check(self.lib.aog_generate_screens(self._handle, int(r[0]), int(r.size), *args))
        else:
            if self._gen is None:
                self._gen = torch.Generator(device=self.device)
                # (one torch stream per instance, offset by the instance's first global env id: distinct atmospheres on every rank,
                # but — unlike 'device' and 'numpy' — not invariant to how the batch is split)
                self._gen.manual_seed(self._base_seed + self.global_env_offset)
            psi = screens_torch(self.num_envs, p.num_pupil_pixels, p.pupil_pixel, self.Cn_squared, p.outer_scale,
                                self.device, self._gen, self.screen_oversampling)   # (Cn_squared: scalar, or [B] per env)
            if mask is None:
                self.set_screens(psi)
            else:
                for e in np.flatnonzero(sel):
                    self.set_screens(psi[e:e + 1], first=int(e))

    def _upload_layer(self, layer):
        torch = self._torch
        self._layer = layer  # keep the host arrays alive during the call
        lt = _lib.AogLayerTables(
            int(layer["stencil_vertical"].size), int(layer["stencil_horizontal"].size),
            _dptr(layer["stencil_vertical"], C.c_int32), _dptr(layer["stencil_horizontal"], C.c_int32),
            _dptr(layer["A_vertical"], C.c_double), _dptr(layer["B_vertical"], C.c_double),
            _dptr(layer["A_horizontal"], C.c_double), _dptr(layer["B_horizontal"], C.c_double),
            float(np.sqrt(self._cn2_table)), float(self.params.pupil_pixel), float(self.params.delta_t))
        _lib.check(self.lib.aog_upload_layer(self._handle, C.byref(lt)))
        v = torch.from_numpy(np.ascontiguousarray(self.velocity_vectors)).to(self.device)
        _lib.check(self.lib.aog_set_wind(self._handle, C.c_void_p(v.data_ptr()), float(np.abs(self.velocity_vectors).max()), self._stream()))
        self._seed_library(draw=False, provisional=True)
        torch.cuda.current_stream(self.device).synchronize()
        self._upload_composite(layer)

    def _upload_composite(self, layer):
        """The step's shifts along each axis as ONE operator (``extrusion_host.compose_extrusions``) for the int8 matrix-core extrusion
        (``aog_upload_layer_composite``).  k_max = the largest whole-pixel shift any env makes per step; winds that would need more than 8
        shifts per axis and step (or ``extrusion='f64'``) keep the float64 round kernels."""
        from .extrusion_host import compose_extrusions

        self.extrusion_kmax = 0
        vmax = float(np.abs(self.velocity_vectors).max()) if self.velocity_vectors.size else 0.0
        k_need = int(np.floor(vmax * self.params.delta_t / self.params.pupil_pixel)) + 1
        if self._extrusion == "f64" or k_need > 8 or os.environ.get("AOG_EXTRUDE_F64"):
            return
        N = self.num_pupil_pixels
        keep = []
        self.extrusion_union = {}     # axis -> [U_1 .. U_kmax]: union stencil sizes of the operators the library cuts out of the uploaded one
        for axis, (st, A, B) in enumerate(((layer["stencil_vertical"], layer["A_vertical"], layer["B_vertical"]),
                                            (layer["stencil_horizontal"], layer["A_horizontal"], layer["B_horizontal"]))):
            yx, Ak, Bk = compose_extrusions(st, A, B, N, k_need, vertical=axis == 0)
            yx, Ak, Bk = np.ascontiguousarray(yx, dtype=np.int32), np.ascontiguousarray(Ak), np.ascontiguousarray(Bk)
            keep.append((yx, Ak, Bk))
            first_use = np.full(yx.size, k_need + 1)
            for j in range(k_need, 0, -1):
                first_use[np.abs(Ak[(j - 1) * N:j * N]).sum(axis=0) > 0] = j
            self.extrusion_union[axis] = [int((first_use <= k).sum()) for k in range(1, k_need + 1)]
            op = _lib.AogLayerComposite(axis, k_need, int(yx.size), 0, _dptr(yx, C.c_int32), _dptr(Ak, C.c_double), _dptr(Bk, C.c_double))
            _lib.check(self.lib.aog_upload_layer_composite(self._handle, C.byref(op)))
        self.extrusion_kmax = k_need

    def set_extrusion_mode(self, mode):
        """'auto' (default: the int8 composite form when its operators were uploaded) | 'f64' (the float64 round kernels: validation form)."""
        _lib.check(self.lib.aog_set_extrusion_mode(self._handle, _lib.AOG_EXTRUDE[mode]))

    def _upload_shack_hartmann(self):
        """shack_hartmann_init (AO_env.py:396-465): host calibration, then the tables of the device chain."""
        from .sh_host import ShackHartmannHost

        sh = ShackHartmannHost(self.params, self.tables)
        self.sh = sh
        c = np.ascontiguousarray
        keep = dict(slot=c(sh.sub_slot, dtype=np.int32), cen=c(sh.centres, dtype=np.float64), ref=c(sh.slopes_ref, dtype=np.float64),
                    rec=c(sh.reconstruction, dtype=np.float64),
                    mla=c(np.stack([sh.mla_phase.real, sh.mla_phase.imag], axis=-1), dtype=np.float64),
                    tf=c(np.stack([sh.transfer.real, sh.transfer.imag], axis=-1), dtype=np.float64), xd=c(sh.x_det, dtype=np.float64))
        t = _lib.AogShTables(int(sh.n_sub), _dptr(keep["slot"], C.c_int32), _dptr(keep["cen"], C.c_double), _dptr(keep["ref"], C.c_double),
                             _dptr(keep["rec"], C.c_double), _dptr(keep["mla"], C.c_double), _dptr(keep["tf"], C.c_double),
                             _dptr(keep["xd"], C.c_double), float(sh.amp_wfs / sh.mag), float(sh.pitch ** 2 * self.params.delta_t), 0.3, 0.01,
                             int(self.sh_fft_precision == "double"), 0)
        _lib.check(self.lib.aog_upload_sh(self._handle, C.byref(t)))

    def SH_step(self):
        """AOEnv.SH_step (AO_env.py:254-290) for every env: returns (actions [B, A] float64 = deformable_mirror_shack.actuators,
        torch.tensor([1])).  Photon noise comes from the handle's Philox stream, or — in host-RNG (parity) mode — from each env's
        numpy stream through hcipy's large_poisson draw order."""
        torch = self._torch
        if not self.SH_operation:
            raise RuntimeError("SH_step needs SH_operation=True (AO_env.py:67-68 only initialises the sensor then)")
        B, N = self.num_envs, self.num_pupil_pixels
        action = torch.empty((B, self.num_modes), dtype=torch.float64, device=self.device)
        if self._host_rng:
            lam = self.sh_image().cpu().numpy()
            noisy = np.empty_like(lam)
            for e in range(B):
                r = self._env_rng(e)
                large = lam[e] > 1e6
                out = np.zeros(N * N)
                out[large] = np.round(lam[e][large] + r.normal(size=int(large.sum())) * np.sqrt(lam[e][large]))
                out[~large] = r.poisson(lam[e][~large], size=int((~large).sum()))
                noisy[e] = out
            nd = torch.from_numpy(noisy).to(self.device)
            _lib.check(self.lib.aog_sh_update(self._handle, C.c_void_p(nd.data_ptr()), C.c_void_p(action.data_ptr()), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()
        else:
            _lib.check(self.lib.aog_sh_image(self._handle, None, self._stream()))
            _lib.check(self.lib.aog_sh_update(self._handle, None, C.c_void_p(action.data_ptr()), self._stream()))
        return action, torch.tensor([1])

    def sh_image(self):
        """Noise-free Shack-Hartmann camera image of every env, [B, N*N] float64 (camera.read_out(), AO_env.py:274)."""
        torch = self._torch
        img = torch.empty((self.num_envs, self.num_pupil_pixels ** 2), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.aog_sh_image(self._handle, C.c_void_p(img.data_ptr()), self._stream()))
        return img

    def sh_update(self, noisy_image):
        """Estimator + leaky integrator on a caller-supplied (already noisy) image [B, N*N] float64 -> actions [B, A] float64.
        ``None``: photon noise from the handle's Philox stream on the image of the last ``sh_image()`` call (what ``SH_step`` does)."""
        torch = self._torch
        action = torch.empty((self.num_envs, self.num_modes), dtype=torch.float64, device=self.device)
        if noisy_image is None:
            nd_ptr = None
        else:
            nd = torch.as_tensor(noisy_image, device=self.device).to(torch.float64).reshape(self.num_envs, -1).contiguous()
            nd_ptr = C.c_void_p(nd.data_ptr())
        _lib.check(self.lib.aog_sh_update(self._handle, nd_ptr, C.c_void_p(action.data_ptr()), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        return action

    def _sh_call(self, who, g_image, g_slopes, actuators, mask, want_grad, want_values):
        """The checks, buffers and the one ``aog_sh_gradient`` call behind ``sh_clean`` and ``sh_gradient``: (grad, image, slopes)."""
        torch = self._torch
        if not self.SH_operation:
            raise ValueError(f"{who}: this environment was built without the Shack-Hartmann sensor (SH_operation=True)")
        B, A, N2, ns = self.num_envs, self.num_modes, self.num_pupil_pixels ** 2, int(self.sh.n_sub)
        arg = lambda x, shape, name: self._f64_arg(x, shape, who, name)
        gi, gs, act = arg(g_image, (B, N2), "g_image"), arg(g_slopes, (B, 2 * ns), "g_slopes"), arg(actuators, (B, A), "actuators")
        mptr, _keep = (None, None)
        if mask is not None:
            _keep = torch.from_numpy(_mask_array(mask, B, who).astype(np.uint8)).to(self.device)
            mptr = C.c_void_p(_keep.data_ptr())
        if want_grad:
            self._upload_gradient()   # (handles on the separable propagation contract with the output gradient's modes operands)
        grad = torch.zeros((B, A), dtype=torch.float64, device=self.device) if want_grad else None
        image = torch.zeros((B, N2), dtype=torch.float64, device=self.device) if want_values else None
        slopes = torch.zeros((B, 2 * ns), dtype=torch.float64, device=self.device) if want_values else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.aog_sh_gradient(self._handle, mptr, ptr(gi), ptr(gs), ptr(act), ptr(grad), ptr(image), ptr(slopes), self._stream()))
        return grad, image, slopes

    def sh_clean(self, actuators=None, mask=None):
        """The CLEAN Shack-Hartmann image [B, N*N] and slopes [B, 2 n_sub] (all s_x, then all s_y: the centroids of the noise-free image
        minus lenslet centres and reference slopes, what the integrator of ``sh_update`` would see without photon noise) with the sensor's
        mirror at its own actuators or at ``actuators`` [B, A]: the forward half of ``sh_gradient`` alone.  Draws no noise and changes
        nothing ``SH_step`` / ``sh_image`` / ``sh_update`` read.  ``mask``: the rows of the envs it leaves out read zero."""
        _, image, slopes = self._sh_call("sh_clean", None, None, actuators, mask, False, True)
        return image, slopes

    def sh_gradient(self, g_image=None, g_slopes=None, actuators=None, mask=None, with_values=False):
        """Vector-Jacobian product of the Shack-Hartmann sensor's clean image and slopes (``aog_sh_gradient``): the gradient of
        ``L = sum(g_image * image) + sum(g_slopes * slopes)`` (cotangents [B, N*N] and [B, 2 n_sub]; ``None`` = zero, at least one given)
        with respect to the sensor mirror's actuators (per metre of surface), a float64 device tensor [B, A].  ``actuators`` [B, A]:
        evaluate there instead of at ``deformable_mirror_shack.actuators`` (never written).  ``mask``: the rows of the envs it leaves out
        read zero.  ``with_values=True`` returns ``(grad, image, slopes)``.  Photon noise is not differentiated: the call draws nothing
        and leaves the noise stream, the integrator and everything a step reads alone.  Pupils of 128, 256, 512, 240 and 480 pixels in
        complex64 run two register-resident backward passes; other envs hipFFT on the padded grid.  Stream-ordered; raises like
        ``pyramid_gradient`` while an action is pending and between two steps of a lookahead episode."""
        if g_image is None and g_slopes is None:
            raise ValueError("sh_gradient: at least one of g_image and g_slopes must be given")
        grad, image, slopes = self._sh_call("sh_gradient", g_image, g_slopes, actuators, mask, True, with_values)
        return (grad, image, slopes) if with_values else grad

    def _host_extrusion_noise(self):
        """Host-RNG (parity) mode: draw the normals of the coming step's extrusions from each env's numpy stream in hcipy's
        order (all x shifts, then all y shifts; ``normal(0, 1, N)`` per extrusion) and hand them to the library."""
        N = self.num_pupil_pixels
        t_prev, t_new = self.timestep * self.delta_t, (self.timestep + 1) * self.delta_t
        shifts = integer_shifts(self.velocity_vectors, t_prev, t_new, self.params.pupil_pixel)  # [B, 2]
        counts = np.abs(shifts).sum(axis=1)
        max_ext = int(counts.max()) if counts.size else 0
        if max_ext == 0:
            return
        noise = np.zeros((self.num_envs, max_ext, N))
        for e in range(self.num_envs):
            r = self._env_rng(e)
            for k in range(int(counts[e])):
                noise[e, k] = r.normal(0, 1, size=N)
        self.set_extrusion_noise(noise)

    def set_extrusion_noise(self, noise):
        """Standard normals for the extrusions of the NEXT ``step`` (dynamic atmosphere, parity runs): ``[B, max_ext, N]`` float64
        device tensor, row k of env b = the ``normal(0, 1, N)`` draw of its k-th extrusion in hcipy's order (x shifts first, then
        y).  Without this call the step draws from the handle's Philox stream."""
        torch = self._torch
        n = torch.as_tensor(noise, device=self.device).to(torch.float64).contiguous()
        if n.dim() != 3 or n.shape[0] != self.num_envs or n.shape[2] != self.num_pupil_pixels:
            raise ValueError("set_extrusion_noise: expected [num_envs, max_ext, N]")
        self._noise_dev = n   # kept alive until the step has run
        _lib.check(self.lib.aog_set_extrusion_noise(self._handle, C.c_void_p(n.data_ptr()), int(n.shape[1]), self._stream()))

    def evolve_atmosphere(self):
        """The atmosphere half of ``step`` and nothing else (``aog_evolve_atmosphere``; dynamic atmosphere only): the clock advances one
        ``delta_t`` and the wind extrusion brings the screens there — after k calls ``get_screens()`` is bit for bit that of a same-seed twin
        stepped k times.  Host-RNG mode draws the step's normals from the envs' numpy streams first, as ``step`` does.  The layers of a
        ``layered.LayeredAOEnv`` advance through this."""
        if self.atm_type != "dynamic":
            raise RuntimeError("evolve_atmosphere: only a dynamic atmosphere evolves between steps")
        if self._host_rng:
            self._host_extrusion_noise()
        _lib.check(self.lib.aog_evolve_atmosphere(self._handle, self._stream()))
        self.timestep += 1
        self.state_epoch += 1

    def install_layer_sum(self, layers):
        """Install the float64 sum of the current screens of ``layers`` (1 .. 8 dynamic ``BatchedAOEnv`` of this env's batch, pupil and
        device) as this quasi-static env's screens (``aog_install_layer_sum``): aperture mean removed, stream-ordered, no host
        synchronisation.  Actuators and counters stay; the next ``reset`` / ``step`` observes the new screens."""
        self._install_layers(self.lib.aog_install_layer_sum, layers)

    def _install_layers(self, entry, layers, *lead, terms=False, coeff=None, coeff_optional=False):
        """The one call behind ``install_layer_sum``, ``LayeredAOEnv.install_layer_sum_disturbed`` and ``layered.install_layer_sum_sightline``:
        ``entry(handle, layer handles, L, *lead[, coeff, K], stream)`` on this env's stream.  ``terms``: the entry point takes coefficients,
        a [B, K] float64 device tensor (None only where ``coeff_optional``: no terms)."""
        who, tail = entry.__name__[len("aog_"):], []
        if terms and coeff is None and coeff_optional:
            tail = [None, 0]
        elif terms:
            torch = self._torch
            if not isinstance(coeff, torch.Tensor) or coeff.dtype != torch.float64 or coeff.dim() != 2 or coeff.shape[0] != self.num_envs or not coeff.is_contiguous():
                raise ValueError(f"{who}: coeff must be a contiguous float64 [{self.num_envs}, K] device tensor")
            tail = [C.c_void_p(coeff.data_ptr()), int(coeff.shape[1])]
        handles = (C.c_void_p * len(layers))(*[lay._handle.value for lay in layers])
        _lib.check(entry(self._handle, handles, len(layers), *lead, *tail, self._stream()))
        self.state_epoch += 1

    def lookahead(self, enable=True):
        """Dynamic atmosphere, device random stream: let every ``step`` launch the NEXT step's wind extrusion on a stream of the library's
        own, beside its epilogue and the caller's policy query (``aog_set_lookahead``).  Same results bit for bit; between two steps of an
        episode ``reset`` / ``get_screens`` / ``get_state`` / ``phase_screen`` / ``focal_image(s)`` / ``sh_image`` raise (the screens already
        stand at the next step) — at episode boundaries they work as ever.  Opt-in (``rollout(lookahead=True)``, ``bench.py --config 4
        --lookahead``): measured on ROCm 7.2 the two cross-stream event hand-offs cost ~20 us each, which is what the overlap saves."""
        if self.atm_type != "dynamic" or self._host_rng:
            return False
        _lib.check(self.lib.aog_set_lookahead(self._handle, int(bool(enable))))
        return bool(enable)

    def set_screen_method(self, screen_method):
        """Switch the device screen synthesis between 'twoband' and 'hcipy16' (``aog_set_screen_method``); takes effect at the next
        regeneration (semi_dynamic ``reset``).  The workspace of the method that is no longer used is given back then."""
        if screen_method not in _lib.AOG_SCREENS:
            raise ValueError("screen_method must be 'twoband' or 'hcipy16'")
        _lib.check(self.lib.aog_set_screen_method(self._handle, _lib.AOG_SCREENS[screen_method]))
        self.screen_method = screen_method

    def device_bytes(self):
        """Bytes of HBM the library handle owns right now (``aog_info.device_bytes``)."""
        _lib.check(self.lib.aog_get_info(self._handle, C.byref(self.info)))
        return int(self.info.device_bytes)

    def get_screens(self, first=0, count=None):
        """Current achromatic screens (hcipy's ``layer._achromatic_screen``: phase * lambda) of envs [first, first + count), default
        all: [count, N, N] float64.  Dynamic atmosphere: the float64 master screens.  Otherwise the stored screen exactly as the step
        kernels read it (aperture pixels only, aperture mean removed)."""
        torch = self._torch
        N = self.num_pupil_pixels
        count = self.num_envs - first if count is None else int(count)
        out = torch.empty((count, N, N), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.aog_get_screens_f64(self._handle, C.c_void_p(out.data_ptr()), int(first), count, self._stream()))
        return out

    def set_screens(self, screens, first=0):
        """Install achromatic screens (hcipy's ``layer._achromatic_screen``: phase * lambda) for envs
        [first, first + len(screens)).  numpy or torch, float32 or float64, shape [k, N, N] or [k, N*N]."""
        torch = self._torch
        if isinstance(screens, np.ndarray):
            screens = torch.from_numpy(np.ascontiguousarray(screens))
        N = self.num_pupil_pixels
        screens = screens.reshape(-1, N, N)
        if screens.dtype not in (torch.float32, torch.float64):
            screens = screens.to(torch.float64)
        screens = screens.to(self.device).contiguous()
        fn = self.lib.aog_set_screens_f64 if screens.dtype == torch.float64 else self.lib.aog_set_screens_f32
        _lib.check(fn(self._handle, C.c_void_p(screens.data_ptr()), int(first), int(screens.shape[0]), self._stream()))
        self.state_epoch += 1
        # the kernel is stream-ordered; keep the source alive until it has run
        torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------------------------------------------------------
    def reset(self, mask=None, seed=None, options=None):
        """AOEnv.reset (AO_env.py:74-103) for every env (or those selected by ``mask``).  ``seed``/``options`` are
        accepted and ignored exactly like the reference.  Returns (obs [B, o^2] float16, {})."""
        m = None if mask is None else self._torch.as_tensor(mask, device=self.device).to(self._torch.uint8).contiguous()
        if self.atm_type == "semi_dynamic":
            self._generate_screens(mask=m)  # layer.reset() (AO_env.py:76-77)
        obs, obs_raw = self._obs_buffers(m is not None)
        _lib.check(self.lib.aog_reset(self._handle, C.c_void_p(m.data_ptr()) if m is not None else None,
                                      C.c_void_p(obs_raw.data_ptr()), C.c_void_p(obs.data_ptr()), self._stream()))
        self._observed(obs, obs_raw)
        if self.servo is not None and self.flat_mirror_start_per_episode:
            self.servo.reset(m)   # (the mirror starts flat, and so does the history of its commands)
        return obs, {}

    _PIPELINE_END = object()
    # counts every change of the state output_gradient reads (reset, step, set_actuators, set_screens, set_state): autograd.step_outputs
    # refuses a backward pass once it has moved
    state_epoch = 0
    _last_action = None
    _last_step = None   # the last step's return tuple; None after a reset
    _gradient_uploaded = False

    def step(self, actions, out=None, next_actions=_PIPELINE_END):
        """AOEnv.step (AO_env.py:106-153).  ``actions``: [B, A] float32 tensor on the device.
        ``next_actions`` (optional; callers that know the next action already — open-loop sequences, replays, synthetic benchmarks):
        a [B, A] float32 device tensor = the actions of the NEXT call, or None on the last step of such a sequence.  The step then goes
        through ``aog_step_pipelined``: identical results, one kernel launch less per step; between two calls of a sequence the mirror
        already holds the next action, so ``reset`` / ``get_state`` / ``focal_images`` ... raise until the sequence is ended with
        ``next_actions=None``.
        Returns (obs float16 [B, o^2], reward float32 [B], done bool [B], trunc bool [B] (all False),
        {"power": [B] float32, "obs_raw": [B, o^2] float32, "strehl": [B] float32}).
        An env built with ``servo=`` steps with ``applied = servo.apply(actions)`` — what the mirror receives this frame after the loop's
        latency, the mirror's response, its stroke and its stuck actuators (``servo.MirrorServo``) — and returns it as
        ``info["applied_action"]`` [B, A] float32; ``next_actions`` is refused there (``RuntimeError``).
        ``out`` (optional): (obs float16 [B, o^2], reward float32 [B], done bool/uint8 [B]) contiguous device tensors to write
        into — a rollout hands in slices of its transition buffers, so nothing is copied afterwards."""
        a = self._as_actions(actions)
        if next_actions is not BatchedAOEnv._PIPELINE_END:
            self._refuse_with_servo("step(next_actions=...)", "step(actions), one call per step")
        if self.atm_type == "dynamic" and self._host_rng:
            self._host_extrusion_noise()
        cached = self._persistent_out and out is None
        if cached and self._step_cache is not None:
            # persistent outputs: the views of the block and their addresses are made once (a step's host cost drops from ~22 to ~10 us, which
            # matters right after a synchronisation, when the first launches of a burst cost the host twice their steady-state time)
            ret, ptrs = self._step_cache
        else:
            ret, ptrs = self._step_outputs(out)
            if cached:
                self._step_cache = (ret, ptrs)
        if self.servo is not None:
            # (last before the launch: a call refused above — a bad ``out``, say — has pushed no frame into the servo's history.  A new
            # tensor per step: _last_action and info["applied_action"] keep it)
            a = ret[4]["applied_action"] = self.servo.apply(a)
        self._launch_step(a, next_actions, ptrs)
        self._last_action = a   # (output_gradient(wrt="action") differentiates through it)
        self._last_step = ret   # (SPGDController.action reads its metric)
        self._observed(ret[0], ret[4]["obs_raw"], step=True)
        return ret

    def _observed(self, obs, obs_raw, step=False):
        """Bookkeeping after the launches of a reset or (``step``) a step that wrote the observation ``obs`` / ``obs_raw``.  Every such call
        goes through here: ``observation_frames`` must follow the library's own count of them (the frame of the detector's random stream,
        which ``get_state`` / ``set_state`` and split batches rely on)."""
        self.last_obs_raw = obs_raw
        self._last_obs = obs
        self.observation_frames += 1
        self.state_epoch += 1
        if not step:
            self._last_action = None
            self._last_step = None
        if step:
            self.timestep += 1

    def _step_outputs(self, out):
        """The tensors a step writes and returns: (step tuple, their addresses in aog_step's order)."""
        torch = self._torch
        n = self.obs_dim ** 2
        B = self.num_envs
        # ONE allocation per step: fp32 block (obs_raw | reward | power | strehl), fp16 obs, uint8 done — or none at all when the
        # caller asked for a persistent block (``persistent_outputs``: the single-env wrapper copies it to the host in one transfer)
        nb32, nb16 = 4 * B * (n + 3), 2 * B * n
        pack = self._pack if self._persistent_out else None
        if pack is None:
            pack = torch.empty((nb32 + nb16 + B,), dtype=torch.uint8, device=self.device)
            if self._persistent_out:
                self._pack = pack
        f32 = pack[:nb32].view(torch.float32)
        obs_raw = f32[: B * n].view(B, n)
        power = f32[B * (n + 1): B * (n + 2)]
        strehl = f32[B * (n + 2):]
        if out is None:
            reward = f32[B * n: B * (n + 1)]
            obs = pack[nb32:nb32 + nb16].view(torch.float16).view(B, n)
            done = pack[nb32 + nb16:]
        else:
            obs, reward, done = out
            ok = (obs.dtype == torch.float16 and tuple(obs.shape) == (B, n) and reward.dtype == torch.float32 and tuple(reward.shape) == (B,)
                  and done.dtype in (torch.bool, torch.uint8) and tuple(done.shape) == (B,)
                  and obs.is_contiguous() and reward.is_contiguous() and done.is_contiguous())
            if not ok:
                raise ValueError("step(out=...): expected contiguous (float16 [B, o^2], float32 [B], bool/uint8 [B]) device tensors")
        base = f32.data_ptr()
        ptrs = (base, obs.data_ptr(), reward.data_ptr(), done.data_ptr(), base + 4 * B * (n + 1), base + 4 * B * (n + 2))
        if self._trunc is None:
            self._trunc = torch.zeros((B,), dtype=torch.bool, device=self.device)
        ret = (obs, reward, done if done.dtype == torch.bool else done.view(torch.bool), self._trunc, {"power": power, "obs_raw": obs_raw, "strehl": strehl})
        return ret, ptrs

    # ------------------------------------------------------------------------------------------------
    # causal policy stepping: the rollout's actor.get_action(obs) -> env.step(action) (algorithm.py:256-262) with the policy attached
    def _policy_net(self, policy, cov_var, policy_out, ou_noise=None, action_mode="sample"):
        """(aog_actor of the policy's next query, (action, log_prob, mean) output tensors, aog_action_noise or None) for the fused tail
        (aog_reset_act / aog_step_act, their _noise forms when ``ou_noise`` or ``action_mode`` differ from the defaults)."""
        from .rollout import action_noise

        torch = self._torch
        noise = action_noise(ou_noise, action_mode)
        if ou_noise is not None:
            ou_noise.check(self.num_envs, self.num_modes, self.device)
        if int(policy.env_id_base) != self.global_env_offset:
            raise ValueError(f"policy.env_id_base ({policy.env_id_base}) != env.global_env_offset ({self.global_env_offset}): the policy's random "
                             "streams are keyed by the global env id of row 0")
        layers = policy.layers()
        S, A = layers[0].weight.shape[1], layers[3].weight.shape[0]
        if S != self.obs_dim ** 2 or A != self.num_modes:
            raise ValueError(f"the actor maps {S} -> {A}; this env observes obs_dim^2 = {self.obs_dim ** 2} and takes num_modes = {self.num_modes}")
        B = self.num_envs
        if policy_out is None:
            action = torch.empty((B, A), dtype=torch.float32, device=self.device)
            log_prob = torch.empty((B,), dtype=torch.float32, device=self.device)
            mean = torch.empty((B, A), dtype=torch.float32, device=self.device)
        else:
            action, log_prob, mean = policy_out
        for t, shape, required in ((action, (B, A), True), (log_prob, (B,), True), (mean, (B, A), False)):
            if (t is None and required) or (t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()
                                                               or t.device != self.device)):
                raise ValueError("policy_out: expected contiguous float32 (action [B, A], log_prob [B], mean [B, A] or None) tensors on the env's device")
        return policy.net(B, cov_var, layers), (action, log_prob, mean), noise

    def _reset_with_tail(self, fn, first, rest):
        """The launches and bookkeeping of a whole-batch ``reset()`` whose last launch also runs a tail (a policy query, an SPGD reset) that
        loads the first action into the mirror: ``fn(handle, first, obs_raw, obs, *rest, stream)``.  The caller has refused a mask and
        checked the tail's arguments.  Returns ``(obs, info)``."""
        if self.atm_type == "semi_dynamic":
            self._generate_screens(mask=None)  # layer.reset() (AO_env.py:76-77)
        obs, obs_raw = self._obs_buffers(False)
        _lib.check(fn(self._handle, first, C.c_void_p(obs_raw.data_ptr()), C.c_void_p(obs.data_ptr()), *rest, self._stream()))
        self._observed(obs, obs_raw)
        return obs, {}

    def _step_with_tail(self, fn, first, a, out, mid, last, keep_last_step):
        """The launches and bookkeeping of a ``step()`` of the pending action (``a`` = None) or of ``a`` whose last launch also runs a tail on
        the new observation, unless the episode ends: ``fn(handle, first, action, the six outputs of aog_step, *mid, &queried, *last, stream)``.
        The caller has checked the tail's arguments.  ``keep_last_step``: the step tuple becomes ``_last_step`` (``SPGDController.action`` reads
        it).  Returns ``(step tuple, whether the tail ran)``."""
        if self.atm_type == "dynamic" and self._host_rng:
            self._host_extrusion_noise()
        ret, ptrs = self._step_outputs(out)
        p = C.c_void_p
        queried = C.c_int(0)
        _lib.check(fn(self._handle, first, p(a.data_ptr() if a is not None else None), p(ptrs[0]), p(ptrs[1]), p(ptrs[2]), p(ptrs[3]), p(ptrs[4]),
                      p(ptrs[5]), *mid, C.byref(queried), *last, self._stream()))
        if keep_last_step:
            self._last_step = ret
        self._observed(ret[0], ret[4]["obs_raw"], step=True)
        return ret, queried.value

    @staticmethod
    def _policy_ptrs(pol, noise):
        """``_policy_net``'s outputs and noise as the library's arguments: ((action, log_prob, mean), (noise,)); noise = NULL is the plain form."""
        p = C.c_void_p
        return ((p(pol[0].data_ptr()), p(pol[1].data_ptr()), p(pol[2].data_ptr() if pol[2] is not None else None)),
                (C.byref(noise) if noise is not None else None,))

    def reset_with_policy(self, policy, cov_var=0.5, policy_out=None, mask=None, ou_noise=None, action_mode="sample"):
        """``reset()`` of the whole batch with ``policy`` (a ``rollout.DeviceActor``) attached (``aog_reset_act``): the reset's last launch
        also queries the policy on the reset observation and loads the resulting action into the mirror, so the next ``step_with_policy``
        steps it (pass no ``action`` there).  Returns ``((obs, info), (action, log_prob, mean))``; the query consumes one of the policy's call
        indices, exactly like ``policy(obs)``.  ``policy_out``: (action [B, A], log_prob [B], mean [B, A] or None) float32 tensors to write
        into.  Masked resets are not fused (the query covers the whole batch): use ``reset(mask)`` and pass the first action.
        ``ou_noise`` (a ``rollout.DeviceOUNoise`` of [B, A]) / ``action_mode="mean"``: the query's action form, as in ``DeviceActor.__call__``
        (``aog_reset_act_noise``)."""
        self._refuse_with_servo("reset_with_policy", "reset() and step(policy(obs)), or rollout(fused_policy=False)")
        if mask is not None:
            raise ValueError("reset_with_policy resets the whole batch; reset some envs with reset(mask) and step with an explicit action")
        net, pol, noise = self._policy_net(policy, cov_var, policy_out, ou_noise, action_mode)
        ptrs, noise = self._policy_ptrs(pol, noise)
        ret = self._reset_with_tail(self.lib.aog_reset_act_noise, C.byref(net), ptrs + noise)
        policy.calls += 1
        return ret, pol

    def step_with_policy(self, policy, cov_var=0.5, out=None, policy_out=None, action=None, ou_noise=None, action_mode="sample"):
        """``step()`` with ``policy`` (a ``rollout.DeviceActor``) attached (``aog_step_act``): steps the action left pending by
        ``reset_with_policy`` or the previous call (``action=None``), or ``action`` (first step after a plain ``reset``; an error while one
        is pending).  Unless this is the episode's last step, the step's last launch also queries the policy on the new observation and
        loads that action into the mirror for the next call: one launch where ``step`` + ``policy(obs)`` + the next ``step``'s prologue take
        three.  Bit-identical to that unfused loop.  Returns ``(step tuple, (action, log_prob, mean))``, or ``(step tuple, None)`` on the
        episode's last step (no query, no call index consumed, ``policy_out`` untouched).  ``out`` as in ``step``; ``policy_out`` as in
        ``reset_with_policy``; ``ou_noise`` / ``action_mode`` as there (``aog_step_act_noise``: the OU state advances only when the policy is
        queried)."""
        self._refuse_with_servo("step_with_policy", "step(policy(obs)), or rollout(fused_policy=False)")
        a = self._as_actions(action) if action is not None else None
        net, pol, noise = self._policy_net(policy, cov_var, policy_out, ou_noise, action_mode)
        ptrs, noise = self._policy_ptrs(pol, noise)
        ret, queried = self._step_with_tail(self.lib.aog_step_act_noise, C.byref(net), a, out, ptrs, noise, keep_last_step=False)
        if not queried:
            return ret, None
        policy.calls += 1
        return ret, pol

    # SPGD stepping: the sensorless baseline's query (sensorless.SPGDController) in the policy's place
    def _spgd_checked(self, ctrl, action_out, who):
        torch = self._torch
        if getattr(ctrl, "env", None) is not self:
            raise ValueError(f"{who}: the controller was built for another env")
        B, A = self.num_envs, self.num_modes
        if action_out is None:
            return torch.empty((B, A), dtype=torch.float32, device=self.device)
        if (action_out.dtype != torch.float32 or tuple(action_out.shape) != (B, A) or not action_out.is_contiguous() or action_out.device != self.device):
            raise ValueError(f"{who}: action_out must be a contiguous float32 [B, A] tensor on the env's device")
        return action_out

    def reset_with_spgd(self, ctrl, mask=None, action_out=None):
        """``reset()`` of the whole batch with ``ctrl`` (a ``sensorless.SPGDController`` of this env) attached (``aog_reset_spgd``): the
        reset's last launch also resets the controller (``ctrl.reset()``: flat start or the env's actuators, iteration counters kept) and
        loads its first command into the mirror, so the next ``step_with_spgd`` steps it (pass no ``action`` there).  Returns
        ``((obs, info), action)``.  Masked resets are not fused: use ``reset(mask)`` + ``ctrl.reset(mask)`` and pass the action."""
        self._refuse_with_servo("reset_with_spgd", "reset(), ctrl.reset() and step(action), or rollout(fused_policy=False)")
        if mask is not None:
            raise ValueError("reset_with_spgd resets the whole batch; reset some envs with reset(mask) + ctrl.reset(mask) and step with an explicit action")
        action = self._spgd_checked(ctrl, action_out, "reset_with_spgd")
        return self._reset_with_tail(self.lib.aog_reset_spgd, ctrl._handle, (C.c_void_p(action.data_ptr()),)), action

    def step_with_spgd(self, ctrl, out=None, action=None, action_out=None):
        """``step()`` with ``ctrl`` attached (``aog_step_spgd``): steps the action left pending by ``reset_with_spgd`` or the previous call
        (``action=None``), or ``action`` (first step after a plain ``reset``).  Unless this is the episode's last step, the step's last launch
        also runs the SPGD query on the metric it has just stored and loads the next command into the mirror: one launch where ``step`` +
        ``ctrl.action()`` + the next ``step``'s prologue take three, bit-identical to that unfused loop.  Returns ``(step tuple, action)``, or
        ``(step tuple, None)`` on the episode's last step (no query, controller and ``action_out`` untouched).  ``out`` as in ``step``, or a
        dict ``{"obs", "reward", "done"}`` of those tensors that may also carry ``"action"`` (= ``action_out``)."""
        self._refuse_with_servo("step_with_spgd", "step(ctrl.action()), or rollout(fused_policy=False)")
        if isinstance(out, dict):
            action_out = out.get("action", action_out)
            out = (out["obs"], out["reward"], out["done"])
        a = self._as_actions(action) if action is not None else None
        nxt = self._spgd_checked(ctrl, action_out, "step_with_spgd")
        ret, queried = self._step_with_tail(self.lib.aog_step_spgd, ctrl._handle, a, out, (C.c_void_p(nxt.data_ptr()),), (), keep_last_step=True)
        return ret, (nxt if queried else None)

    def _as_actions(self, actions):
        """[B, A] float32 contiguous device tensor (as is when it already is one)."""
        torch = self._torch
        if (isinstance(actions, torch.Tensor) and actions.dtype == torch.float32 and actions.device == self.device and actions.is_contiguous()
                and actions.dim() == 2 and actions.shape[0] == self.num_envs and actions.shape[1] == self.num_modes):
            return actions
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.float32:
            a = a.to(torch.float32)
        return a.reshape(self.num_envs, self.num_modes).contiguous()

    def _launch_step(self, a, next_actions, ptrs):
        p = C.c_void_p
        pending = self._next_actions_keepalive
        if next_actions is BatchedAOEnv._PIPELINE_END:
            self._next_actions_keepalive = None
            _lib.check(self.lib.aog_step(self._handle, p(a.data_ptr()), p(ptrs[0]), p(ptrs[1]), p(ptrs[2]), p(ptrs[3]), p(ptrs[4]), p(ptrs[5]),
                                         self._stream()))
        else:
            # continuation of a pipelined sequence: the mirror already holds what the PREVIOUS call announced as next_actions and the library
            # ignores `actions` — a caller that passes something else (a corrected action, say) would silently get the old one's results
            if pending is not None and a is not pending and not (a.data_ptr() == pending.data_ptr() and a.shape == pending.shape):
                # (other storage: compared by value, which synchronises — AOG_CHECK_PIPELINE=0 skips it for callers that copy their actions around)
                if os.environ.get("AOG_CHECK_PIPELINE") != "0" and not bool(self._torch.equal(a, pending)):
                    raise ValueError("step(next_actions=...): `actions` differs from the next_actions announced by the previous call of this "
                                     "pipelined sequence (the mirror already holds those); end the sequence with next_actions=None first")
            nxt = None
            if next_actions is not None:
                nxt = self._as_actions(next_actions)
            self._next_actions_keepalive = nxt   # (read by the launch enqueued here; checked against the next call's actions)
            _lib.check(self.lib.aog_step_pipelined(self._handle, p(a.data_ptr()), p(nxt.data_ptr() if nxt is not None else None), p(ptrs[0]),
                                                   p(ptrs[1]), p(ptrs[2]), p(ptrs[3]), p(ptrs[4]), p(ptrs[5]), self._stream()))

    def persistent_outputs(self, enable=True):
        """Write every ``step``'s outputs into ONE block that lives as long as the env instead of fresh tensors: the tensors a step
        returns are then views that the NEXT step overwrites.  For callers that consume a step's outputs before stepping again (the
        single-env wrapper: one device-to-host copy of the block per step); returns the block layout (n = obs_dim^2):
        float32 [B n] obs_raw | [B] reward | [B] power | [B] strehl, then float16 [B n] obs, then uint8 [B] done."""
        self._persistent_out = bool(enable)
        self._step_cache = None
        if not enable:
            self._pack = None
        n, B = self.obs_dim ** 2, self.num_envs
        return {"float32_bytes": 4 * B * (n + 3), "float16_bytes": 2 * B * n, "uint8_bytes": B}

    # ------------------------------------------------------------------------------------------------
    def get_actuators(self):
        """deformable_mirror.actuators of every env, [B, A] float64 (metres)."""
        torch = self._torch
        out = torch.empty((self.num_envs, self.num_modes), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.aog_get_actuators(self._handle, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_actuators(self, act):
        torch = self._torch
        a = torch.as_tensor(act, device=self.device).to(torch.float64).reshape(self.num_envs, self.num_modes).contiguous()
        _lib.check(self.lib.aog_set_actuators(self._handle, C.c_void_p(a.data_ptr()), self._stream()))
        self.state_epoch += 1
        self._last_action = None
        torch.cuda.current_stream(self.device).synchronize()

    def focal_image(self, env_index=0):
        """``wf_wfs_after_foc.electric_field`` of one env (AO_env.py:138): complex64 [n_focal, n_focal] (y, x), up to a global
        phase.  ``abs()**2 * tables.focal_pixel_area`` is the ``.power`` image the reference's render() shows."""
        torch = self._torch
        nf = int(self.tables.focal_m1.shape[0])
        out = torch.empty((nf, nf, 2), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.aog_focal_image(self._handle, int(env_index), C.c_void_p(out.data_ptr()), self._stream()))
        return torch.view_as_complex(out)

    def focal_images(self, first=0, count=None):
        """``wf_wfs_after_foc.electric_field`` (AO_env.py:138) of envs [first, first + count), default all: complex64
        [count, n_focal, n_focal] — the batched form of ``focal_image`` (matrix-core complex GEMM pair, fast precision only)."""
        torch = self._torch
        nf = int(self.tables.focal_m1.shape[0])
        count = self.num_envs - first if count is None else int(count)
        out = torch.empty((count, nf, nf, 2), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.aog_focal_images(self._handle, int(first), count, C.c_void_p(out.data_ptr()), self._stream()))
        return torch.view_as_complex(out)

    def wavefront_truth(self, out=None):
        """Residual wavefront statistics and the best-fit mirror command of every env in its current state (``aog_wavefront_truth``): a dict of
        float64 device tensors ``rms`` [B] (RMS optical path error over the aperture, metres), ``fit_rms`` [B] (what is left of it after the
        best correction the mirror's modes can make: the fitting error), ``coef`` [B, A] (least-squares coefficients of the path error on the
        modes, metres of path) and ``ideal_actuators`` [B, A] (the actuators that remove everything the mirror can reach:
        ``get_actuators() - coef / 2``).  Stream-ordered, no host synchronisation, nothing a step reads is changed.  ``out``: such a dict to
        write into.  The fit's host table (``optics_host.wavefront_fit``) is uploaded by the first call.  Raises like ``focal_images`` while a
        pipelined or policy-attached step has an action pending and between two steps of a lookahead episode."""
        if not self._wavefront_fit_uploaded:
            from .optics_host import wavefront_fit

            modes = np.ascontiguousarray(self.tables.modes, dtype=np.float64)
            fit = np.ascontiguousarray(wavefront_fit(modes), dtype=np.float64)
            _lib.check(self.lib.aog_upload_wavefront_fit(self._handle, modes.ctypes.data_as(C.c_void_p), fit.ctypes.data_as(C.c_void_p)))
            self._wavefront_fit_uploaded = True
        B, A = self.num_envs, self.num_modes
        shapes = {"rms": (B,), "fit_rms": (B,), "coef": (B, A), "ideal_actuators": (B, A)}
        text = "contiguous float64 device tensors rms [B], fit_rms [B], coef [B, A], ideal_actuators [B, A]"
        if out is None:
            out = {k: self._f64_out(None, s, "wavefront_truth", text, zero=False) for k, s in shapes.items()}
        else:
            for k, s in shapes.items():   # (every entry must be there: a missing one is not made here)
                self._f64_out(False if out.get(k) is None else out[k], s, "wavefront_truth", text)
        p = C.c_void_p
        _lib.check(self.lib.aog_wavefront_truth(self._handle, p(out["rms"].data_ptr()), p(out["fit_rms"].data_ptr()), p(out["coef"].data_ptr()),
                                                p(out["ideal_actuators"].data_ptr()), self._stream()))
        return out

    def ideal_action(self):
        """The ideal modal controller's action, [B, A] float64 in the form of ``SH_step()``'s (raw actuators, for an env built with
        ``SH_operation=True``): the actuators that leave only the fitting error on the screen the last observation saw."""
        torch = self._torch
        if not self._wavefront_fit_uploaded:
            return self.wavefront_truth()["ideal_actuators"]
        act = torch.empty((self.num_envs, self.num_modes), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.aog_wavefront_truth(self._handle, None, None, None, C.c_void_p(act.data_ptr()), self._stream()))
        return act

    # ------------------------------------------------------------------------------------------------
    # what the off-step instruments' wrappers share
    # instrument -> (the attribute holding its host tables, what an env without it was built without, its upload method)
    _INSTRUMENTS = {"science": ("_science", "a science camera (science_window=...)", "_upload_science"),
                    "pyramid": ("_pyramid", "a pyramid sensor (pyramid=dict(...))", "_upload_pyramid")}

    def _instrument_mask(self, instrument, mask, who):
        """``who``'s checks on ``instrument`` (built with it; its tables uploaded, on demand), then its mask as a device pointer (None: every
        env) and the tensor that keeps it alive."""
        tables, without, upload = self._INSTRUMENTS[instrument]
        if getattr(self, tables) is None:
            raise ValueError(f"{who}: this environment was built without {without}")
        getattr(self, upload)()
        if mask is None:
            return None, None
        sel = _mask_array(mask, self.num_envs, who)
        m = self._torch.from_numpy(sel.astype(np.uint8)).to(self.device)
        return C.c_void_p(m.data_ptr()), m

    def _f64_arg(self, x, shape, who, name):
        """An input ``x`` (None stays None; numpy, torch on any device, any dtype) as a contiguous float64 tensor on the env's device;
        ValueError unless it has ``shape``."""
        if x is None:
            return None
        t = self._torch.as_tensor(x, device=self.device).to(self._torch.float64)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _f64_out(self, out, shape, who, text, zero=True):
        """An ``out=`` tensor: ``out`` itself if it is a contiguous float64 tensor of ``shape`` on the env's device, a new one (zeros, or
        uninitialised with ``zero=False``) for None, and ``ValueError(f"{who}(out=...): expected {text}")`` for anything else."""
        torch = self._torch
        if out is None:
            return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=torch.float64, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != tuple(shape) or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError(f"{who}(out=...): expected {text}")
        return out

    # ------------------------------------------------------------------------------------------------
    # analytic gradient
    @property
    def obs_gradient(self):
        """True when ``output_gradient`` takes ``g_obs`` on this separable-route env (the ``obs_gradient=True`` keyword; read-only)."""
        return self._obs_gradient

    def _upload_gradient(self):
        """The output gradient's tables to the handle (``aog_upload_gradient`` and, on ``obs_gradient`` envs, ``aog_upload_gradient_obs``);
        no-op when they are there."""
        if self._gradient_uploaded:
            return
        _lib.check(self.lib.aog_upload_gradient(self._handle, C.byref(self._upload_keep[1])))
        if self._obs_gradient:
            _lib.check(self.lib.aog_upload_gradient_obs(self._handle, C.byref(self._obs_mft_keep[2])))
        self._gradient_uploaded = True

    def output_gradient(self, g_obs=None, g_power=None, g_strehl=None, wrt="actuators", action=None, with_values=False):
        """Vector-Jacobian product of the optical outputs at the state the last reset or step left (``aog_output_gradient``): the gradient of
        ``L = sum(g_obs * obs_raw) + sum(g_power * power) + sum(g_strehl * strehl)`` (cotangents: [B, o^2], [B], [B]; ``None`` = zero, at
        least one given) as a float64 device tensor [B, A].  ``wrt="actuators"``: with respect to ``get_actuators()`` (per metre of surface);
        ``wrt="action"``: with respect to the float32 action through the normalisation of AO_env.py:119-120 (``action`` defaults to the last
        action the mirror received: the one passed to ``step()``, or on an env with a servo ``info["applied_action"]`` — the gradient is with
        respect to what the mirror received, not to the command; not on ``SH_operation`` environments, whose action is the actuators).  The atmosphere never depends on
        the action and a step sets the mirror absolutely, so this one-step gradient is the complete derivative of everything step t returns
        with respect to the policy.  The observation noise of ``set_detector`` does not enter: the gradient is of the clean outputs.
        ``with_values=True`` returns ``(grad, values)`` with ``values`` [B, o^2 + 2] the float64 obs_raw, power and Strehl the gradient was
        taken at.  On the separable observation route (``obs_dim`` 6 .. 32; float64 envs from 8) the observation is a matrix Fourier transform and
        its gradient is opt-in: an env made with ``obs_gradient=True`` (``aog_upload_gradient_obs``) takes ``g_obs`` and returns the float64
        ``obs_raw`` in ``values``; without it ``g_obs`` is refused there and the observation entries of ``values`` are NaN, while power and
        Strehl have their gradients either way.  The Strehl reward is the Strehl itself
        (AO_env.py:476-487); callers chain the SSIM reward themselves.  Stream-ordered, no host synchronisation, nothing a step reads is
        changed; ``wrt=None`` (with ``with_values=True``) runs the forward half alone and returns ``(None, values)``; raises like
        ``wavefront_truth`` while an action is pending and between two steps of a lookahead episode."""
        torch = self._torch
        if wrt not in ("actuators", "action", None):
            raise ValueError("output_gradient: wrt must be 'actuators' or 'action' (or None with with_values=True: the values alone)")
        if wrt is None and not with_values:
            raise ValueError("output_gradient: wrt=None asks for the values alone and needs with_values=True")
        self._upload_gradient()
        B, A, n = self.num_envs, self.num_modes, self.obs_dim ** 2
        cot = lambda x, shape, name: self._f64_arg(x, shape, "output_gradient", name)
        go, gp, gs = cot(g_obs, (B, n), "g_obs"), cot(g_power, (B,), "g_power"), cot(g_strehl, (B,), "g_strehl")
        a = None
        if wrt == "action":
            a = self._last_action if action is None else self._as_actions(action)
            if a is None:
                raise ValueError("output_gradient(wrt='action'): no action given and no step() taken since the last reset")
        grad = torch.empty((B, A), dtype=torch.float64, device=self.device) if wrt is not None else None
        values = torch.empty((B, n + 2), dtype=torch.float64, device=self.device) if with_values else None
        p = C.c_void_p
        ptr = lambda t: p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.aog_output_gradient(self._handle, ptr(go), ptr(gp), ptr(gs), ptr(a), ptr(grad) if wrt == "actuators" else None,
                                                ptr(grad) if wrt == "action" else None, ptr(values), self._stream()))
        return (grad, values) if with_values else grad

    # ------------------------------------------------------------------------------------------------
    # science camera
    def _upload_science(self):
        """The camera's host tables to the handle (``aog_upload_science``); no-op without ``science_window`` or when they are there."""
        t = self._science
        if t is None or self._science_uploaded:
            return
        m1 = np.ascontiguousarray(np.stack([t.m1.real, t.m1.imag], axis=-1), dtype=np.float64)
        m2 = np.ascontiguousarray(np.stack([t.m2.real, t.m2.imag], axis=-1), dtype=np.float64)
        bins = np.ascontiguousarray(t.ee_bin, dtype=np.int32)
        _lib.check(self.lib.aog_upload_science(self._handle, m1.ctypes.data_as(C.c_void_p), m2.ctypes.data_as(C.c_void_p), int(t.window),
                                               float(t.phase_ratio), float(t.peak_fraction), bins.ctypes.data_as(C.c_void_p), int(t.radii.size)))
        self._science_uploaded = True

    def science_integrate(self, mask=None):
        """Add the current science-arm frame of every env (or those ``mask`` selects) to its long exposure (``aog_science_integrate``).
        Stream-ordered; reads the state the last ``reset`` / ``step`` left and changes nothing a step reads.  Raises like ``focal_images``
        while a pipelined or policy-attached step has an action pending and between two steps of a lookahead episode."""
        ptr, _keep = self._instrument_mask("science", mask, "science_integrate")   # (the mask lives until the launches are queued: torch frees in stream order)
        _lib.check(self.lib.aog_science_integrate(self._handle, ptr, self._stream()))

    def science_clear(self, mask=None):
        """Empty the long exposure (and frame count) of every env, or of those ``mask`` selects."""
        ptr, _keep = self._instrument_mask("science", mask, "science_clear")
        _lib.check(self.lib.aog_science_clear(self._handle, ptr, self._stream()))

    def science_exposure(self, first=0, count=None, image=True):
        """The long exposures of envs [first, first + count), default all, as a dict of device tensors: ``psf`` [count, w, w] float64 the
        mean frame (``image=False``: left out), ``strehl`` [count] its centre pixel (the long-exposure Strehl ratio),
        ``encircled_energy`` [count, len(science_radii)] the share of the beam's power inside each of ``science_radii`` (lambda_sci / D),
        ``frames`` [count] int32.  An env with no frames reads as zeros.  A range outside the batch raises ``ValueError``."""
        torch = self._torch
        self._instrument_mask("science", None, "science_exposure")
        first = int(first)
        count = self.num_envs - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.num_envs:
            raise ValueError(f"science_exposure: envs [{first}, {first + count}) lie outside [0, {self.num_envs})")
        w, n_ee = self._science.window, int(self._science.radii.size)
        out = {"strehl": torch.empty((count,), dtype=torch.float64, device=self.device),
               "encircled_energy": torch.empty((count, n_ee), dtype=torch.float64, device=self.device),
               "frames": torch.empty((count,), dtype=torch.int32, device=self.device)}
        if image:
            out["psf"] = torch.empty((count, w, w), dtype=torch.float64, device=self.device)
        p = C.c_void_p
        _lib.check(self.lib.aog_science_read(self._handle, int(first), count, p(out["psf"].data_ptr()) if image else None, p(out["strehl"].data_ptr()),
                                             p(out["encircled_energy"].data_ptr()), p(out["frames"].data_ptr()), self._stream()))
        return out

    # ------------------------------------------------------------------------------------------------
    # modulated pyramid wavefront sensor
    def _upload_pyramid(self):
        """The sensor's host tables to the handle (``aog_upload_pyramid``); no-op without ``pyramid=`` or when they are there."""
        t = self._pyramid
        if t is None or self._pyramid_uploaded:
            return
        from .pyramid_host import packed_operands

        c2 = lambda z: np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), dtype=np.float64)
        keep = dict(m1=c2(t.m1), m2=c2(t.m2), b1=c2(t.b1), b2=c2(t.b2), valid=np.ascontiguousarray(t.valid, dtype=np.int32))
        ops = packed_operands(t)
        keep.update({k: ops[k] for k in ("m1s", "m2s", "b1s", "b2s")})
        p = lambda a: a.ctypes.data
        tabs = _lib.AogPyramidTables(t.samples, t.pixels, t.n_mod, t.n_valid, p(keep["m1"]), p(keep["m2"]), p(keep["b1"]), p(keep["b2"]), p(keep["m1s"]),
                                     p(keep["m2s"]), p(keep["b1s"]), p(keep["b2s"]), p(keep["valid"]), ops["fwd_unscale"], ops["back_unscale"],
                                     float(self.pyramid["photons"] or 0.0))
        _lib.check(self.lib.aog_upload_pyramid(self._handle, C.byref(tabs)))
        self._pyramid_uploaded = True
        self.pyramid_frame_count = 0

    def pyramid_frames(self, mask=None, out=None):
        """The pyramid sensor's frame of every env at the state the last ``reset`` / ``step`` left: [B, 4, n_s, n_s] float64, quadrant
        2 (k_y > 0) + (k_x > 0).  ``mask``: the rows of the envs it leaves out are not written (``out``: the tensor to write into).
        Stream-ordered; changes nothing a step reads.  Raises like ``science_integrate`` while an action is pending and between two steps
        of a lookahead episode."""
        ptr, _keep = self._instrument_mask("pyramid", mask, "pyramid_frames")
        ns = self._pyramid.pixels
        out = self._f64_out(out, (self.num_envs, 4, ns, ns), "pyramid_frames", "a contiguous float64 [B, 4, n_s, n_s] tensor on the env's device")
        _lib.check(self.lib.aog_pyramid_frames(self._handle, ptr, C.c_void_p(out.data_ptr()), self._stream()))
        self.pyramid_frame_count += 1
        return out

    def pyramid_slopes(self, mask=None, out=None):
        """The sensor's slopes [B, 2 n_valid] float64: s_x over the valid pixels (``env._pyramid.valid``), then s_y.  As ``pyramid_frames``."""
        ptr, _keep = self._instrument_mask("pyramid", mask, "pyramid_slopes")
        out = self._f64_out(out, (self.num_envs, 2 * self._pyramid.n_valid), "pyramid_slopes",
                            "a contiguous float64 [B, 2 n_valid] tensor on the env's device")
        _lib.check(self.lib.aog_pyramid_slopes(self._handle, ptr, C.c_void_p(out.data_ptr()), self._stream()))
        self.pyramid_frame_count += 1
        return out

    def pyramid_gradient(self, g_frames=None, g_slopes=None, actuators=None, mask=None, with_values=False):
        """Vector-Jacobian product of the sensor's clean frame and slopes (``aog_pyramid_gradient``): the gradient of
        ``L = sum(g_frames * frame) + sum(g_slopes * slopes)`` (cotangents [B, 4, n_s, n_s] and [B, 2 n_valid]; ``None`` = zero, at least one
        given) with respect to ``get_actuators()`` (per metre of surface), a float64 device tensor [B, A].  ``actuators`` [B, A]: evaluate
        there instead of at the mirror's own (the mirror is not written).  ``mask``: the rows of the envs it leaves out are not written
        (they read as zeros).  ``with_values=True`` returns ``(grad, frames, slopes)`` with the clean frame and slopes at that point.
        Photon noise is not differentiated: the call draws nothing and leaves ``pyramid_frame_count`` alone.  Fast envs run the backward
        pass on the matrix cores (built for ``samples`` <= 32); float64 envs a plain float64 chain per env.  Stream-ordered; raises like ``pyramid_frames`` while an action
        is pending and between two steps of a lookahead episode."""
        torch = self._torch
        if g_frames is None and g_slopes is None:
            raise ValueError("pyramid_gradient: at least one of g_frames and g_slopes must be given")
        if self._pyramid is None:
            raise ValueError("pyramid_gradient: this environment was built without a pyramid sensor (pyramid=dict(...))")
        B, A, ns, nv = self.num_envs, self.num_modes, self._pyramid.pixels, self._pyramid.n_valid
        arg = lambda x, shape, name: self._f64_arg(x, shape, "pyramid_gradient", name)
        gf, gs = arg(g_frames, (B, 4, ns, ns), "g_frames"), arg(g_slopes, (B, 2 * nv), "g_slopes")
        act = arg(actuators, (B, A), "actuators")
        mptr, _keep = self._instrument_mask("pyramid", mask, "pyramid_gradient")
        if self._precision != "fp64":
            self._upload_gradient()   # (fast handles contract with the output gradient's modes operands)
        grad = torch.zeros((B, A), dtype=torch.float64, device=self.device)
        frames = torch.zeros((B, 4, ns, ns), dtype=torch.float64, device=self.device) if with_values else None
        slopes = torch.zeros((B, 2 * nv), dtype=torch.float64, device=self.device) if with_values else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.aog_pyramid_gradient(self._handle, mptr, ptr(gf), ptr(gs), ptr(act), ptr(grad), ptr(frames), ptr(slopes), self._stream()))
        return (grad, frames, slopes) if with_values else grad

    def pyramid_clean(self, actuators=None, mask=None):
        """The CLEAN frames [B, 4, n_s, n_s] and slopes [B, 2 n_valid] (no photon noise, ``pyramid_frame_count`` untouched) at the mirror's
        actuators or at ``actuators`` [B, A]: the forward half of ``pyramid_gradient`` alone.  Returns (frames, slopes)."""
        torch = self._torch
        if self._pyramid is None:
            raise ValueError("pyramid_clean: this environment was built without a pyramid sensor (pyramid=dict(...))")
        B, A, ns, nv = self.num_envs, self.num_modes, self._pyramid.pixels, self._pyramid.n_valid
        act = self._f64_arg(actuators, (B, A), "pyramid_clean", "actuators")
        mptr, _keep = self._instrument_mask("pyramid", mask, "pyramid_clean")
        frames = torch.zeros((B, 4, ns, ns), dtype=torch.float64, device=self.device)
        slopes = torch.zeros((B, 2 * nv), dtype=torch.float64, device=self.device)
        p = C.c_void_p
        _lib.check(self.lib.aog_pyramid_gradient(self._handle, mptr, None, None, p(act.data_ptr()) if act is not None else None, None,
                                                 p(frames.data_ptr()), p(slopes.data_ptr()), self._stream()))
        return frames, slopes

    def pyramid_calibrate(self):
        """Calibrate the reconstructor through the device sensor itself: on a scratch env of 2 A + 1 flat wavefronts (same tables, precision
        and sensor, no photon noise) mode k is pushed and pulled by ``poke`` metres, response[:, k] = (s+ - s-) / (2 poke), the command
        matrix is ``inverse_tikhonov(response, rcond)`` and the reference slopes are the flat wavefront's.  Returns (command matrix
        [A, 2 n_valid], reference slopes [2 n_valid]) as numpy arrays (also ``pyramid_response``); ``PYR_step`` calls it when needed."""
        from .optics_host import inverse_tikhonov

        self._instrument_mask("pyramid", None, "pyramid_calibrate")
        A, N, cfg = self.num_modes, self.num_pupil_pixels, self.pyramid
        sensor = {k: cfg[k] for k in ("samples", "q", "pixels", "n_mod", "r_mod")}
        scratch = BatchedAOEnv(2 * A + 1, self.device, act_type=self.act_type, act_dim=A, obs_dim=self.obs_dim, rew_type=self.rew_type,
                               params=self.params, screens=np.zeros((2 * A + 1, N, N)), precision=self._precision, kernel=self._kernel,
                               tables=self.tables, pyramid=sensor, verbose=False)
        try:
            act = np.zeros((2 * A + 1, A))
            act[1:A + 1] = cfg["poke"] * np.eye(A)
            act[A + 1:] = -cfg["poke"] * np.eye(A)
            scratch.set_actuators(act)
            s = scratch.pyramid_slopes().cpu().numpy()
        finally:
            scratch.close()
        self.pyramid_response = (s[1:A + 1] - s[A + 1:]).T / (2.0 * cfg["poke"])          # [2 n_valid, A]
        recon = np.ascontiguousarray(inverse_tikhonov(self.pyramid_response, cfg["rcond"]), dtype=np.float64)
        ref = np.ascontiguousarray(s[0], dtype=np.float64)
        _lib.check(self.lib.aog_upload_pyramid_reconstructor(self._handle, recon.ctypes.data_as(C.c_void_p), ref.ctypes.data_as(C.c_void_p)))
        self.pyramid_reconstructor, self.pyramid_reference_slopes = recon, ref
        self._pyramid_calibrated = True
        return recon, ref

    def PYR_step(self):
        """The pyramid sensor's integrator, the counterpart of ``SH_step``: one sensor call, then a <- a - gain R (s - s_ref) for every env.
        Returns (actuators [B, A] float64, slopes [B, 2 n_valid] float64); the mirror itself is not touched — step with the actuators
        (an env built with ``SH_operation=True`` takes them as its action)."""
        torch = self._torch
        self._instrument_mask("pyramid", None, "PYR_step")
        if not self._pyramid_calibrated:
            self.pyramid_calibrate()
        act = torch.empty((self.num_envs, self.num_modes), dtype=torch.float64, device=self.device)
        slopes = torch.empty((self.num_envs, 2 * self._pyramid.n_valid), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.aog_pyramid_update(self._handle, float(self.pyramid["gain"]), C.c_void_p(act.data_ptr()), C.c_void_p(slopes.data_ptr()),
                                               self._stream()))
        self.pyramid_frame_count += 1
        return act, slopes

    def phase_screen(self, env_index=0):
        """Atmospheric phase at the sensing wavelength [N, N] float32 radians (0 outside the aperture, aperture mean removed) — the
        quantity render() displays as ``phase_screen_opd`` after scaling by lambda_wfs / (2 pi) * 1e6 (AO_env.py:87-88)."""
        torch = self._torch
        N = self.num_pupil_pixels
        out = torch.empty((N, N), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.aog_get_phase_screen(self._handle, int(env_index), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def get_state(self):
        """Snapshot of the simulation state: ``set_state`` on an env built with the same arguments, or on this one after it has moved on,
        resumes bit-identically — every later observation, reward, ``done``, Strehl, power, screen and instrument reading is that of the
        uninterrupted run.

        In it: the library's blob (screens, or the master screens, ring origins and extrusion counters of a dynamic atmosphere; the
        screen-synthesis counters; mirror and Shack-Hartmann actuators; render times; and in its tail the seed, the Shack-Hartmann call
        count, the steps since the reset, the detector's frame and the pyramid sensor's frame), ``timestep``, ``episode_no``,
        ``observation_frames``, ``pyramid_frame_count``, the Fried parameters, the detector's values and the host RNG streams.

        Deliberately not in it: the science camera's exposure and frame counts (measurement data: ``set_state`` leaves them exactly as
        they were; ``science_clear`` at the snapshot point makes two runs' exposures comparable), the tensor given to
        ``accumulate_returns`` (the caller's) and profiling records.  What belongs to another object is that object's to save: a
        ``rollout.DeviceActor`` and a ``rollout.DeviceOUNoise`` have ``get_state`` / ``set_state`` of their own (the call index and the
        OU state key the exploration streams), like the controllers of ``device_handle``.

        Raises while a pipelined or policy-attached step has an action pending and between two steps of a lookahead episode: take the
        snapshot where nothing is pending (``next_actions=None``, an episode's last step)."""
        torch = self._torch
        n = int(self.lib.aog_state_bytes(self._handle))
        blob = torch.zeros((n,), dtype=torch.uint8, device=self.device)   # (the library pads every part to 256 bytes and leaves the padding alone)
        ts = C.c_int64()
        _lib.check(self.lib.aog_get_state(self._handle, C.c_void_p(blob.data_ptr()), C.byref(ts), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        rng = [self._env_rng(e).get_state() for e in range(self.num_envs)] if self._host_rng else None
        return {"blob": blob, "lib_timestep": int(ts.value), "timestep": self.timestep, "episode_no": self.episode_no, "rng": rng,
                "num_envs": self.num_envs, "fried_parameters": self._fried.copy(),
                "observation_frames": self.observation_frames,
                "detector": None if self._detector is None else {k: v.copy() for k, v in self._detector.items()},
                "pyramid": None if self.pyramid is None else {k: self.pyramid[k] for k in ("samples", "q", "pixels", "n_mod", "r_mod", "photons")},
                "pyramid_frame_count": self.pyramid_frame_count, **({} if self.servo is None else {"servo": self.servo.state_dict()})}

    def _check_servo_state(self, state):
        """``ValueError`` unless ``state`` and this env both have a mirror servo, of one configuration, or neither has; nothing is touched."""
        if ("servo" in state) != (self.servo is not None):
            raise ValueError("set_state: the state was saved " + ("with" if "servo" in state else "without") + " a mirror servo, this environment was "
                             "built " + ("without" if self.servo is None else "with") + " one (servo=dict(...))")
        if self.servo is not None:
            self.servo.check_state_dict(state["servo"])

    def set_state(self, state):
        """Resume from a ``get_state`` snapshot (see there for what it holds and what it leaves alone).  Whatever the handle had pending
        — a pipelined or policy-attached action, a lookahead extrusion, the int8 extrusion's work ahead — is forgotten.  ``ValueError`` for
        a state of another configuration: another ``num_envs``, a detector or a pyramid sensor on one side only."""
        torch = self._torch
        # every refusal comes before the handle is touched (blobs of different num_envs can have one size: their parts are padded to 256 bytes)
        fried = state.get("fried_parameters")
        saved_envs = state.get("num_envs", None if fried is None else np.asarray(fried).shape[0])
        if saved_envs is not None and int(saved_envs) != self.num_envs:
            raise ValueError(f"set_state: the state was saved with num_envs = {int(saved_envs)} and this environment has {self.num_envs}")
        det = state.get("detector")
        if (det is None) != (self._detector is None):
            raise ValueError("set_state: the state was saved " + ("without" if det is None else "with") + " a detector and this environment was built "
                             + ("with" if det is None else "without") + " one (obs_photons)")
        if "pyramid" in state and (state["pyramid"] is None) != (self.pyramid is None):   # (states from before the sensor was saved: no rule)
            raise ValueError("set_state: the state was saved " + ("without" if state["pyramid"] is None else "with") + " a pyramid sensor and this "
                             "environment was built " + ("with" if state["pyramid"] is None else "without") + " one (pyramid=dict(...))")
        self._check_servo_state(state)
        if det is not None and any(np.asarray(det[k]).shape != (self.num_envs,) for k in ("photons", "read_noise", "background")):
            raise ValueError("state's detector values do not match this environment's num_envs")
        blob = state["blob"].to(self.device).contiguous()
        if blob.numel() != int(self.lib.aog_state_bytes(self._handle)):
            raise ValueError("state blob does not match this environment's configuration")
        if self.servo is not None:
            self.servo.load_state_dict(state["servo"])   # (ValueError for a servo of another configuration, before the handle is touched)
        self._upload_pyramid()   # (no-op when the sensor is there: an upload AFTER the restore would restart the frame count the blob brings)
        _lib.check(self.lib.aog_set_state(self._handle, C.c_void_p(blob.data_ptr()), int(state["lib_timestep"]), self._stream()))
        self.state_epoch += 1
        self._last_action = None
        torch.cuda.current_stream(self.device).synchronize()
        self._next_actions_keepalive = None   # (the library forgot a pending pipelined action: the next step's is not checked against it)
        self.timestep = int(state["timestep"])
        self.episode_no = int(state["episode_no"])
        self.observation_frames = int(state.get("observation_frames", 0))   # (the library's own count came with the blob)
        self.pyramid_frame_count = int(state.get("pyramid_frame_count", 0))   # (likewise)
        if state.get("rng") is not None:
            for e, st in enumerate(state["rng"]):
                self._env_rng(e).set_state(st)
        if fried is not None and not np.array_equal(np.asarray(fried, dtype=np.float64), self._fried):
            self._apply_fried(fried)   # (the values only: the screens came with the blob)
        if det is not None:
            self._detector = {k: np.ascontiguousarray(det[k], dtype=np.float64).copy() for k in ("photons", "read_noise", "background")}
            self._push_detector()   # (the frame count came with the blob)

    def accumulate_returns(self, returns=None):
        """Have every ``step`` add its rewards into ``returns`` ([B] float32 contiguous device tensor; the caller zeroes it at
        episode start) inside the step's last kernel — the episode-return sum of the rollout without a launch of its own.
        ``None`` detaches.  The tensor must stay alive while attached (a reference is kept here)."""
        if not self._handle:   # closed env (or one whose construction failed): nothing to attach to or detach from
            self._returns_ref = None
            return
        torch = self._torch
        if returns is not None:
            ok = returns.dtype == torch.float32 and tuple(returns.shape) == (self.num_envs,) and returns.is_contiguous() and returns.is_cuda
            if not ok:
                raise ValueError("accumulate_returns: expected a contiguous float32 [num_envs] tensor on the env's device")
        self._returns_ref = returns
        _lib.check(self.lib.aog_set_return_accumulator(self._handle, C.c_void_p(returns.data_ptr() if returns is not None else None)))

    def device_status(self):
        """Synchronise and return the library's sticky device status word (0 = fine)."""
        v = C.c_int32()
        _lib.check(self.lib.aog_device_status(self._handle, C.byref(v)))
        return int(v.value)

    def profile(self, enable=True, every=1, block=8):
        """HIP-event timing of the fused kernel; ``every`` = n times one block of ``block`` consecutive launches in n (the records hold the
        stream ~6 us per timed launch)."""
        _lib.check(self.lib.aog_profile_block(self._handle, int(block)))
        _lib.check(self.lib.aog_profile_enable(self._handle, max(1, int(every)) if enable else 0))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int()
        _lib.check(self.lib.aog_profile_read(self._handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_kernels(self):
        """{name: (mean ms, launches)} of every kernel id timed since profiling was switched on, as collected by the LAST ``profile_read()``
        (``_lib.AOG_PROF``: screen synthesis passes, screen packing, extrusion, Shack-Hartmann passes; HIP events on the launch stream)."""
        out = {}
        for name, kid in _lib.AOG_PROF.items():
            ms, n = C.c_double(), C.c_int()
            _lib.check(self.lib.aog_profile_read_kernel(self._handle, kid, C.byref(ms), C.byref(n)))
            if n.value:
                out[name] = (ms.value, n.value)
        return out

    def close(self):
        h, self._handle = self._handle, None
        if h:
            self.lib.aog_destroy(h)
        servo, self.servo = self.__dict__.get("servo"), None
        if servo is not None:
            servo.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
