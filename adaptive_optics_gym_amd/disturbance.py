"""Vibration and static aberrations on top of the layered atmosphere.

Turbulence is not all that perturbs a real wavefront: telescope and terminal jitter puts narrow spectral lines on tip and tilt, and every
bench carries a static non-common-path error.  ``ModalDisturbance`` holds K <= 8 fixed pupil shapes and, per env and shape, a
coefficient = a static offset + a damped oscillator driven by white noise, sampled at the frame time (an AR(2) process generated on the
device: ``aog_disturbance_*``, ``csrc/k_disturbance.h``).  ``LayeredAOEnv(..., disturbance=dict(...))`` advances it once per step and adds
``sum_k coeff[b][k] shape_k`` inside the float64 sum of the layers it installs (``aog_install_layer_sum_disturbed``), so everything that
reads the front's screens sees it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .device_handle import DeviceHandle, ptr
from .params import resolve_per_env

MAX_TERMS = _lib.DISTURBANCE_MAX_TERMS
SHAPES = ("tip", "tilt", "focus")
PARAMETERS = ("a1", "a2", "b", "sigma", "rho1")


def ar2_parameters(frequency, damping, rms, delta_t):
    """The AR(2) process x_t = a1 x_{t-1} + a2 x_{t-2} + b n_t (n_t standard normal) of a damped oscillator of natural frequency
    ``frequency`` f0 (Hz) and damping ratio ``damping`` zeta sampled every ``delta_t`` seconds, scaled to the stationary standard deviation
    ``rms``: r = exp(-zeta 2 pi f0 dt), theta = 2 pi f0 sqrt(1 - zeta^2) dt, a1 = 2 r cos(theta), a2 = -r^2,
    b = rms sqrt((1 + a2)((1 - a2)^2 - a1^2) / (1 - a2)); also sigma = rms and rho1 = a1 / (1 - a2), the lag-1 correlation the stationary
    start needs.  Returns dict(a1, a2, b, sigma, rho1).  ``ValueError`` unless 0 < zeta < 1, 0 < f0 < 1 / (2 dt) and rms >= 0 (rms = 0: the
    term stays at its static offset)."""
    f0, zeta, rms, dt = float(frequency), float(damping), float(rms), float(delta_t)
    if not (math.isfinite(dt) and dt > 0):
        raise ValueError(f"delta_t must be positive and finite (got {delta_t!r})")
    if not 0.0 < zeta < 1.0:
        raise ValueError(f"damping must lie in (0, 1) (got {damping!r})")
    if not 0.0 < f0 < 0.5 / dt:
        raise ValueError(f"frequency must lie in (0, {0.5 / dt} Hz), below the Nyquist frequency of the frame rate (got {frequency!r})")
    if not (math.isfinite(rms) and rms >= 0.0):
        raise ValueError(f"rms must be finite and >= 0 (got {rms!r})")
    r = math.exp(-zeta * 2.0 * math.pi * f0 * dt)
    theta = 2.0 * math.pi * f0 * math.sqrt(1.0 - zeta * zeta) * dt
    a1, a2 = 2.0 * r * math.cos(theta), -r * r
    b = rms * math.sqrt((1.0 + a2) * ((1.0 - a2) ** 2 - a1 ** 2) / (1.0 - a2))
    return dict(a1=a1, a2=a2, b=b, sigma=rms, rho1=a1 / (1.0 - a2))


def named_shape(name, x_ap, y_ap):
    """``"tip"`` (x), ``"tilt"`` (y) or ``"focus"`` (x^2 + y^2) at the aperture pixels, aperture mean removed, unit RMS over the aperture."""
    x, y = np.asarray(x_ap, dtype=np.float64), np.asarray(y_ap, dtype=np.float64)
    if name not in SHAPES:
        raise ValueError(f"shapes: a shape is one of {SHAPES} or an [N, N] array (got {name!r})")
    v = {"tip": x, "tilt": y, "focus": x * x + y * y}[name]
    v = v - v.mean()
    return v / np.sqrt(np.mean(v * v))


def resolve_shapes(shapes, tables, N):
    """``shapes`` as [K, n_ap] float64 at the packed aperture pixels: names (``named_shape`` on the env's own pupil grid), [N, N] arrays, or
    one [K, N, N] array (taken as they are: a coefficient of 1 m puts the array's values, in metres of optical path, on the wavefront)."""
    if isinstance(shapes, str):
        shapes = [shapes]
    if isinstance(shapes, np.ndarray) and shapes.ndim == 2:
        shapes = shapes[None]
    rows = []
    for s in shapes:
        if isinstance(s, str):
            rows.append(named_shape(s, tables.x_ap, tables.y_ap))
            continue
        a = np.asarray(s, dtype=np.float64)
        if a.shape != (N, N):
            raise ValueError(f"shapes: an explicit shape is an [{N}, {N}] array on the pupil grid (got shape {a.shape})")
        rows.append(a.ravel()[np.asarray(tables.ap_index)])
    if not 1 <= len(rows) <= MAX_TERMS:
        raise ValueError(f"shapes: 1 .. {MAX_TERMS} shapes (got {len(rows)})")
    basis = np.ascontiguousarray(np.stack(rows), dtype=np.float64)
    if not np.all(np.isfinite(basis)):
        raise ValueError("shapes: every value on the aperture must be finite")
    return basis


def resolve_terms(K, vibrations, static, delta_t, num_envs, total_envs, global_env_offset):
    """The generator's parameters as a dict of [B, K] float64 arrays (a1, a2, b, sigma, rho1, offset).  ``vibrations``: dicts with exactly the
    keys term, frequency, damping, rms — at most one per term; frequency, damping and rms are scalars or per-env values under
    ``params.resolve_per_env``'s rules.  ``static``: None, [K] or [num_envs, K] metres of optical path."""
    B = int(num_envs)
    out = {k: np.zeros((B, K)) for k in PARAMETERS + ("offset",)}
    seen = set()
    for v in vibrations or ():
        if not isinstance(v, dict) or set(v) != {"term", "frequency", "damping", "rms"}:
            raise ValueError("vibrations: every entry is a dict with exactly the keys 'term', 'frequency', 'damping' and 'rms'")
        k = int(v["term"])
        if not 0 <= k < K or k in seen:
            raise ValueError(f"vibrations: term {v['term']!r} must name one of the {K} shapes, each at most once")
        seen.add(k)
        cols = [resolve_per_env(f"vibrations[{k}].{name}", v[name], B, total_envs, global_env_offset)[0] for name in ("frequency", "damping", "rms")]
        for e in range(B):
            p = ar2_parameters(cols[0][e], cols[1][e], cols[2][e], delta_t)
            for name in PARAMETERS:
                out[name][e, k] = p[name]
    if static is not None:
        s = np.asarray(static, dtype=np.float64)
        if s.shape not in ((K,), (B, K)) or not np.all(np.isfinite(s)):
            raise ValueError(f"static: expected finite values of shape [{K}] or [{B}, {K}] (got shape {s.shape})")
        out["offset"][:] = s
    return out


class ModalDisturbance(DeviceHandle):
    """The modal disturbance of ``env`` (a ``LayeredAOEnv``, or any ``BatchedAOEnv`` for its pupil grid, batch, global env ids and device).

    shapes       ``"tip"``, ``"tilt"``, ``"focus"`` (built on the env's own pupil grid, unit RMS over the aperture) and / or explicit [N, N]
                 arrays; K <= 8 in all (``resolve_shapes``).
    vibrations   a list of dict(term, frequency, damping, rms): term k's coefficient oscillates at ``frequency`` Hz with damping ratio
                 ``damping`` and standard deviation ``rms`` metres of optical path (``ar2_parameters``); scalars or per-env values.
    static       [K] or [B, K] metres of optical path: the non-common-path aberration, constant in time.
    seed         of the normals (default: the env's); they are keyed by the GLOBAL env id and a call counter, so instances that hold the
                 parts of a batch and make the same calls reproduce the whole batch bit for bit.

    ``advance(mask=None, noise_out=None)`` moves the selected envs one frame on and returns the coefficients [B, K] float64 (metres);
    ``coefficients()`` returns them as they stand; ``reset(mask=None)`` draws the selected envs' stationary start anew (the constructor
    has drawn everyone's); ``state_dict()`` / ``load_state_dict()`` resume bit-identically.  ``basis`` [K, n_ap] holds the shapes at the
    packed aperture pixels, ``basis_master`` the same in the unit of the master screens (2 pi x metres), which is what a front takes
    (``upload_basis(front)``)."""

    prefix, noun = "aog_disturbance", "disturbance"

    def __init__(self, env, shapes, vibrations=(), static=None, seed=None):
        import torch

        self.num_envs, self.global_env_offset = int(env.num_envs), int(env.global_env_offset)
        self.basis = resolve_shapes(shapes, env.tables, int(env.num_pupil_pixels))
        self.n_terms = int(self.basis.shape[0])
        self.basis_master = np.ascontiguousarray(2.0 * np.pi * self.basis)
        self.params = resolve_terms(self.n_terms, vibrations, static, float(env.delta_t), self.num_envs, int(env.total_envs), self.global_env_offset)
        self.seed = int(env._base_seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self._bind(torch, env.device, self.num_envs)
        self._create()
        host = [np.ascontiguousarray(self.params[k]).ctypes.data_as(C.c_void_p) for k in PARAMETERS + ("offset",)]
        self._call("set_params", *host)
        self.coeff = torch.zeros((self.num_envs, self.n_terms), dtype=torch.float64, device=self.device)
        self.reset()

    def _config(self):
        return _lib.AogDisturbanceConfig(_lib.ABI_VERSION, self.num_envs, self.n_terms, self.global_env_offset, self.seed)

    def _noise(self, noise_out, shape, who):
        if noise_out is None:
            return None
        return self._tensor(noise_out, shape, self._torch.float64, f"{who}: noise_out must be a contiguous float64 {list(shape)} tensor on {self.device}")

    def reset(self, mask=None, noise_out=None):
        """The stationary start of the selected envs (all without a mask); ``noise_out`` [B, K, 2] receives the two normals of each."""
        n = self._noise(noise_out, (self.num_envs, self.n_terms, 2), "reset")
        self._call("reset", ptr(self._mask(mask, "reset")), ptr(n), self._stream())

    def advance(self, mask=None, noise_out=None):
        """One frame on for the selected envs; returns ``coeff`` [B, K] float64 (the instance's own buffer, rewritten by every call)."""
        n = self._noise(noise_out, (self.num_envs, self.n_terms), "advance")
        self._call("advance", ptr(self._mask(mask, "advance")), ptr(self.coeff), ptr(n), self._stream())
        return self.coeff

    def coefficients(self):
        """The coefficients as they stand, offset + vibration: [B, K] float64 metres of optical path (the instance's own buffer)."""
        self._call("coefficients", ptr(self.coeff), self._stream())
        return self.coeff

    def upload_basis(self, front):
        """Hand ``basis_master`` to the quasi-static env ``front`` (``aog_upload_disturbance_basis``: a blocking copy)."""
        _lib.check(self.lib.aog_upload_disturbance_basis(front._handle, self.basis_master.ctypes.data_as(C.c_void_p), self.n_terms))

    def state_dict(self):
        return {"blob": self.get_state(), "num_envs": self.num_envs, "n_terms": self.n_terms}

    def load_state_dict(self, state):
        if int(state.get("num_envs", -1)) != self.num_envs or int(state.get("n_terms", -1)) != self.n_terms:
            raise ValueError(f"load_state_dict: the state is of another disturbance (this one: {self.num_envs} envs, {self.n_terms} terms)")
        self.set_state(state["blob"])
