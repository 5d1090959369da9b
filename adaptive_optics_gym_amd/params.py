"""Every constant the reference environment fixes (``parameters_init``, AO_env.py:197-251), as a typed
dataclass instead of the reference's ``exec``-injected dict.  ``num_pupil_pixels`` is the one new knob:
the reference hard-codes 240 (AO_env.py:216); BASELINE.json's configs use 128/256/512."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class OpticalParams:
    telescope_diameter: float = 0.5                 # AO_env.py:213
    num_pupil_pixels: int = 240                     # AO_env.py:216
    wavelength_wfs: float = 1.5e-6                  # AO_env.py:219
    wavelength_sci: float = 2.2e-6                  # AO_env.py:220
    delta_t: float = 1e-3                           # AO_env.py:226
    outer_scale: float = 10.0                       # AO_env.py:230
    D_pupil_fiber: float = 0.5                      # AO_env.py:233
    num_pupil_pixels_fiber: int = 128               # AO_env.py:234 (effectively unused)
    num_focal_pixels_fiber: int = 128               # AO_env.py:235
    multimode_fiber_core_radius: float = 25 * 1e-6  # AO_env.py:237
    singlemode_fiber_core_radius: float = 4.5 * 1e-6  # AO_env.py:238
    fiber_NA: float = 0.14                          # AO_env.py:239
    fiber_length: float = 10.0                      # AO_env.py:240
    f_number: float = 50.0                          # AO_env.py:243
    num_lenslets: int = 12                          # AO_env.py:244
    sh_diameter: float = 5e-3                       # AO_env.py:245
    stellar_magnitude: float = -5.0                 # AO_env.py:246
    focal_q: int = 4                                # AO_env.py:314
    focal_num_airy: int = 30                        # AO_env.py:314
    action_rms_fraction: float = 0.1                # AO_env.py:120  (0.1 * wavelength_sci)
    ssim_ref_peak: float = 2.8                      # AO_env.py:492
    ssim_alpha: float = 0.8                         # AO_env.py:497

    @property
    def fiber_focal_length(self) -> float:          # AO_env.py:388
        return self.D_pupil_fiber / (2 * self.fiber_NA)

    @property
    def fiber_window(self) -> float:                # AO_env.py:381
        return 2.1 * self.multimode_fiber_core_radius

    @property
    def pupil_pixel(self) -> float:
        return self.telescope_diameter / self.num_pupil_pixels


def coerce_velocity(atm_type: str, velocity_value, verbose: bool = True):
    """AO_env.py:200-208 — same coercions, same printed messages."""
    if atm_type in ("quasi_static", "semi_dynamic") and velocity_value != 0:
        if verbose:
            print("In " + atm_type + " atmospheric condition, the velocity value should be zero.")
            print("therefore velocity value is changed to zero")
        velocity_value = 0
    elif atm_type == "dynamic" and velocity_value == 0:
        if verbose:
            print("In " + atm_type + " atmospheric condition, the velocity value cannot be zero.")
            print("therefore velocity value is changed to 1 m/s")
        velocity_value = 1
    return velocity_value


def resolve_per_env(name: str, value, num_envs: int, total_envs: int, global_env_offset: int):
    """A per-env argument (``atm_fried``, ``atm_vel``) as (local [num_envs] float64 array, the array it was cut from, is_scalar).

    ``value``: a scalar (every env), ``num_envs`` values (this instance's envs) or ``total_envs`` values indexed by GLOBAL env id and sliced
    at ``global_env_offset`` — so the instances holding the slices of one batch see the values one instance holding all of it sees.
    Non-finite entries and wrong lengths raise ``ValueError``; the range checks are the caller's."""
    arr = np.asarray(value, dtype=np.float64)
    if arr.ndim == 0:
        if not np.isfinite(arr):
            raise ValueError(f"{name} must be finite, got {value!r}")
        full = np.full(num_envs, float(arr))
        return full, full, True
    if arr.ndim != 1 or arr.size not in (num_envs, total_envs):
        raise ValueError(f"{name}: expected a scalar or a 1-D array of num_envs ({num_envs}) or total_envs ({total_envs}) values, "
                         f"got shape {arr.shape}")
    if not np.all(np.isfinite(arr)):
        raise ValueError(f"{name} must be finite")
    whole = arr.copy()
    if arr.size == num_envs:
        return whole, whole, False
    return whole[global_env_offset:global_env_offset + num_envs].copy(), whole, False


def resolve_detector(photons, read_noise, background, num_envs: int, total_envs: int, global_env_offset: int):
    """The photodetector arguments (``obs_photons``, ``obs_read_noise``, ``obs_background``), each a scalar, ``num_envs`` or ``total_envs``
    values like ``atm_fried`` (``resolve_per_env``), checked: ``None`` when ``photons`` is None (no detector: the noise-free observation),
    else dict(photons, read_noise, background), [num_envs] float64 arrays.  ``ValueError`` for non-finite values, photons <= 0, negative
    read noise or background, wrong lengths; ``None`` for read_noise / background means 0."""
    if photons is None:
        return None
    out = {}
    for key, name, value in (("photons", "obs_photons", photons), ("read_noise", "obs_read_noise", read_noise),
                             ("background", "obs_background", background)):
        local, whole, _ = resolve_per_env(name, 0.0 if value is None else value, num_envs, total_envs, global_env_offset)
        if key == "photons":
            if np.any(whole <= 0):
                raise ValueError("obs_photons: photo-electrons per frame must be > 0")
        elif np.any(whole < 0):
            raise ValueError(f"{name} must be >= 0")
        out[key] = np.ascontiguousarray(local, dtype=np.float64)
    return out


def coerce_velocities(atm_type: str, speeds, verbose: bool = True):
    """``coerce_velocity`` applied to every entry of a [B] float64 array of wind speeds (AO_env.py:200-208).  Each message the reference
    prints is printed once when at least one entry was changed."""
    speeds = np.asarray(speeds, dtype=np.float64)
    if np.any(speeds < 0):
        raise ValueError("atm_vel: wind speeds must be >= 0")
    out = np.array([float(coerce_velocity(atm_type, float(v), False)) for v in speeds], dtype=np.float64)
    if verbose and np.any(out != speeds) and speeds.size:
        first = int(np.flatnonzero(out != speeds)[0])
        coerce_velocity(atm_type, float(speeds[first]), True)
    return out


def resolve_turbulence(atm_type: str, atm_fried, atm_vel, num_envs: int, total_envs: int, global_env_offset: int, verbose: bool = True):
    """The constructor's per-env turbulence arguments, checked and coerced: dict(fried [num_envs], fried_all (the array the values were cut
    from: the whole batch's when total_envs values were given), fried_scalar, speeds [num_envs] after coercion, velocity (what
    ``coerce_velocity`` returns for a scalar, else the speeds), vel_scalar).  ``ValueError`` for non-finite values, r0 <= 0, speeds < 0
    and wrong lengths."""
    fried, fried_all, fried_scalar = resolve_per_env("atm_fried", atm_fried, num_envs, total_envs, global_env_offset)
    if np.any(fried_all <= 0) or np.any(fried <= 0):
        raise ValueError("atm_fried: Fried parameters must be > 0")
    speeds, _, vel_scalar = resolve_per_env("atm_vel", atm_vel, num_envs, total_envs, global_env_offset)
    if np.any(speeds < 0):
        raise ValueError("atm_vel: wind speeds must be >= 0")
    if vel_scalar:
        velocity = coerce_velocity(atm_type, atm_vel, verbose)
        speeds = np.full(num_envs, float(velocity))
    else:
        speeds = coerce_velocities(atm_type, speeds, verbose)
        velocity = speeds.copy()
    return dict(fried=fried, fried_all=fried_all, fried_scalar=fried_scalar, speeds=speeds, velocity=velocity, vel_scalar=vel_scalar)
