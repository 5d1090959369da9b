"""Altitude-conjugated deformable mirrors: the corrector that acts on angular anisoplanatism.

A mirror conjugated to the altitude of a turbulent layer is seen displaced by ``h x angle`` along a line of sight, exactly as the layer
is, so the beacon and the uplink of a ``LayeredAOEnv`` read different footprints of the same surface — which is what lets a controller do
better off axis than "ideal on the beacon" (MCAO; in a link terminal a high-altitude corrector for the uplink).  ``AltitudeMirror`` is
that mirror as a device object (``aog_altmirror_*``, ``csrc/k_conjugate.h``, ``include/aogym_conjugate.h``): a [B, K] command becomes a
[B, M, M] float64 surface on the meta-pupil (``set_command``), the installation of the layer sum reads the surfaces beside the layers
(``install_layer_sum_conjugate``), and ``fit_layer`` gives the best-fit command of a layer's current screen, the ceiling an MCAO
controller is read against.  ``LayeredAOEnv(altitude_mirrors=[...])`` owns such mirrors and installs them on every front.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device_handle import DeviceHandle, ptr

MAX_MODES = _lib.ALTMIRROR_MAX_MODES
MAX_SOURCES = 8   # aog_install_layer_sum_conjugate's limit on layers + mirrors


def influence_basis(n_pixels, actuators=9, coupling=0.15):
    """[K, M, M] float64, K = actuators^2: Gaussian influence functions of an ``actuators x actuators`` grid spread across the M-grid (the
    outer actuators on its edge pixels, pitch d = (M - 1) / (actuators - 1)); actuator (j, i) is mode j actuators + i.  The value at the
    neighbouring actuator is ``coupling``, the peak 2 pi: one metre of optical path per unit command, in the unit of the master screens
    (phase x lambda = 2 pi x metres).  ``ValueError`` for actuators outside 1 .. 16 or coupling outside (0, 1)."""
    M, n = int(n_pixels), int(actuators)
    if n != actuators or not 1 <= n * n <= MAX_MODES:
        raise ValueError(f"actuators: an integer in 1 .. 16 (at most {MAX_MODES} modes), got {actuators!r}")
    if not 0.0 < float(coupling) < 1.0:
        raise ValueError(f"coupling: the influence function's value at the neighbouring actuator, in (0, 1), got {coupling!r}")
    if M < 1:
        raise ValueError(f"n_pixels must be >= 1, got {n_pixels!r}")
    centres = np.linspace(0.0, M - 1.0, n) if n > 1 else np.array([(M - 1) / 2.0])
    pitch = (M - 1.0) / (n - 1) if n > 1 and M > 1 else float(M)
    x = np.arange(M, dtype=np.float64)
    g = np.exp(np.log(float(coupling)) * ((x[None, :] - centres[:, None]) / pitch) ** 2)   # [n, M]: separable
    return np.ascontiguousarray((2.0 * np.pi) * (g[:, None, :, None] * g[None, :, None, :]).reshape(n * n, M, M))


def fit_matrix(basis):
    """[K, M M] float64: the rows of the pseudo-inverse of the basis — ``fit @ screen.ravel()`` is the least-squares command of a screen."""
    b = np.asarray(basis, dtype=np.float64)
    return np.ascontiguousarray(np.linalg.pinv(b.reshape(b.shape[0], -1).T))


def mirror_altitude(spec):
    """The altitude (metres) of one entry of ``altitude_mirrors``, with the checks of the entry's form: ``ValueError`` unless it is a dict
    with 'altitude' (finite, >= 0) and no keys besides 'actuators', 'basis' and 'coupling'."""
    if not isinstance(spec, dict) or "altitude" not in spec or not set(spec) <= {"altitude", "actuators", "basis", "coupling"}:
        raise ValueError("altitude_mirrors: every mirror is a dict with 'altitude' and, optionally, 'actuators' or 'basis', and 'coupling'")
    h = float(spec["altitude"])
    if not np.isfinite(h) or h < 0:
        raise ValueError(f"altitude_mirrors: altitudes must be finite and >= 0, got {spec['altitude']!r}")
    return h


def resolve_mirror(spec, n_pupil, n_meta):
    """One entry of ``altitude_mirrors`` checked: dict(altitude, n_pixels, actuators | basis, coupling).  ``spec``: a dict with 'altitude'
    (metres, finite, >= 0) and either 'actuators' (default 9) with 'coupling' (default 0.15) or 'basis' ([K, M, M]); M is ``n_meta`` for
    an altitude above 0 and ``n_pupil`` on the ground.  ``ValueError`` otherwise; nothing is built."""
    h = mirror_altitude(spec)
    M = int(n_meta) if h > 0 else int(n_pupil)
    out = dict(altitude=h, n_pixels=M, coupling=float(spec.get("coupling", 0.15)))
    if spec.get("basis") is not None:
        if "actuators" in spec:
            raise ValueError("altitude_mirrors: give 'actuators' or 'basis', not both")
        b = np.asarray(spec["basis"], dtype=np.float64)
        if b.ndim != 3 or b.shape[1:] != (M, M) or not 1 <= b.shape[0] <= MAX_MODES or not np.all(np.isfinite(b)):
            raise ValueError(f"altitude_mirrors: basis must be a finite [K, {M}, {M}] array with K in 1 .. {MAX_MODES}, got shape {b.shape}")
        out["basis"] = b
        out["n_modes"] = int(b.shape[0])
    else:
        out["actuators"] = spec.get("actuators", 9)
        influence_basis(1, out["actuators"], out["coupling"])   # (the checks, on the smallest grid)
        out["n_modes"] = int(out["actuators"]) ** 2
    return out


def install_layer_sum_conjugate(front, layers, mirrors, shifts, coeff=None):
    """``layered.install_layer_sum_sightline`` with the surfaces of ``mirrors`` (``AltitudeMirror``, in order) as further sources behind the
    layers (``aog_install_layer_sum_conjugate``): ``shifts`` [L + n_mirrors, B, 2] float64 host array, the layers' first.  Layers plus mirrors
    are at most 8.  Stream-ordered: it reads the surfaces behind a ``set_command`` made on the same stream."""
    n = len(layers) + len(mirrors)
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    if shifts.shape != (n, front.num_envs, 2):
        raise ValueError(f"install_layer_sum_conjugate: shifts must be [{n}, {front.num_envs}, 2], got {shifts.shape}")
    handles = (C.c_void_p * max(1, len(mirrors)))(*[m._handle.value for m in mirrors])
    front._install_layers(front.lib.aog_install_layer_sum_conjugate, layers, handles, len(mirrors), C.c_void_p(shifts.ctypes.data), terms=True, coeff=coeff,
                          coeff_optional=True)


class AltitudeMirror(DeviceHandle):
    """A deformable mirror conjugated to ``altitude`` (metres) over ``env``'s batch and device.

    env        a ``LayeredAOEnv`` built with ``layer_altitudes`` (its ``meta_pupil_pixels`` is the grid of a mirror above the ground), or any
               ``BatchedAOEnv`` for ``altitude == 0`` (the grid is the pupil's N).
    actuators  the default basis: ``influence_basis(M, actuators, coupling)``, K = actuators^2 modes.
    basis      instead of it, [K, M, M] float64: the surface per unit command of each mode, in the master screens' unit.

    ``set_command(cmd, mask=None)`` stores [B, K] float64 commands — metres of optical path with the default basis — for the envs the mask
    selects and synthesises their surfaces (one launch; float64, every product and sum rounded in mode order, so ``tests/conjugate_reference.py``
    replays it bit for bit and an env's surface does not depend on its batch); the other envs keep command and surface.  ``command`` and
    ``surface()`` read them back.  ``fit_layer(l)`` is the best-fit command of layer l's current screen, [B, K] (``pinv`` of the basis applied
    to the layer's logical screen): a mirror at the layer's altitude that takes ``-fit_layer(l)`` cancels as much of the layer as its
    actuators reach, on every sightline at once.  ``get_state()`` / ``set_state()`` carry the commands (a restored mirror has its surfaces
    again).  The mirror is absolute and has no servo: a command stands until it is set again.  Everything runs on the caller's current
    stream."""

    prefix, noun = "aog_altmirror", "altitude mirror"

    def __init__(self, env, altitude, actuators=9, basis=None, coupling=0.15):
        import torch

        spec = dict(altitude=altitude, coupling=coupling)
        spec.update(dict(basis=basis) if basis is not None else dict(actuators=actuators))
        n_meta = getattr(env, "meta_pupil_pixels", None)
        if float(altitude) > 0 and n_meta is None:
            raise ValueError("AltitudeMirror: a mirror above the ground needs an env with layer_altitudes (its meta-pupil is the mirror's grid)")
        plan = resolve_mirror(spec, env.num_pupil_pixels, n_meta if n_meta is not None else env.num_pupil_pixels)
        self._env = env
        self.altitude, self.n_pixels, self.n_modes = plan["altitude"], plan["n_pixels"], plan["n_modes"]
        self.num_envs = int(env.num_envs)
        self.basis = plan["basis"] if "basis" in plan else influence_basis(self.n_pixels, plan["actuators"], plan["coupling"])
        self.fit = fit_matrix(self.basis)
        self._bind(torch, env.device, self.num_envs)
        self._create()
        b, f = (torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (self.basis.reshape(self.n_modes, -1), self.fit))
        self._call("upload", ptr(b), ptr(f), self._stream())
        torch.cuda.current_stream(self.device).synchronize()   # (b and f are temporaries)

    def _config(self):
        return _lib.AogAltMirrorConfig(_lib.ABI_VERSION, self.num_envs, self.n_pixels, self.n_modes, 0)

    def set_command(self, cmd, mask=None):
        """``cmd`` [B, K] (float64 on the device as it is; anything else is converted) becomes the command of the envs ``mask`` selects (all
        without one); their surfaces follow.  Returns the float64 device tensor that was set."""
        torch = self._torch
        c = torch.as_tensor(cmd, device=self.device).to(torch.float64).contiguous()
        if tuple(c.shape) != (self.num_envs, self.n_modes):
            raise ValueError(f"set_command: cmd must be [{self.num_envs}, {self.n_modes}], got {list(c.shape)}")
        self._call("set_command", ptr(c), ptr(self._mask(mask, "set_command")), self._stream())
        return c

    def _get(self, want_surface):
        torch = self._torch
        shape = (self.num_envs, self.n_pixels, self.n_pixels) if want_surface else (self.num_envs, self.n_modes)
        out = torch.empty(shape, dtype=torch.float64, device=self.device)
        self._call("get", *((None, ptr(out)) if want_surface else (ptr(out), None)), self._stream())
        return out

    command = property(lambda self: self._get(False), doc="[B, K] float64: the commands as they stand")

    def surface(self):
        """[B, M, M] float64: the surfaces as they stand, in the master screens' unit."""
        return self._get(True)

    def fit_layer(self, layer):
        """[B, K] float64: the best-fit command of the current screen of layer ``layer`` (an index into the env's layers, or a dynamic
        ``BatchedAOEnv`` of M pixels)."""
        lay = self._env.layers[layer] if isinstance(layer, (int, np.integer)) else layer
        if lay.num_pupil_pixels != self.n_pixels or lay.num_envs != self.num_envs:
            raise ValueError(f"fit_layer: the layer has {lay.num_envs} envs of {lay.num_pupil_pixels} pixels, the mirror {self.num_envs} of {self.n_pixels}")
        out = self._torch.empty((self.num_envs, self.n_modes), dtype=self._torch.float64, device=self.device)
        self._call("fit", lay._handle, ptr(out), self._stream())
        return out
