"""Loop latency and mirror dynamics: the plant between a controller's command and the mirror.

A real loop reads out, computes and converts for one to three frames — often a fraction of a frame more — before the mirror moves; the
mirror then settles in a finite time, its drive range is finite and a few actuators are dead.  ``MirrorServo`` is that plant as a device
model (``aog_servo_*``, ``csrc/k_servo.h``, ``include/aogym_servo.h``): per env a delay line of the commanded actions read ``latency``
frames back (linearly interpolated between two frames for a fractional value), a clip to ``[-stroke, stroke]``, a first-order response
``y += response (c - y)`` and, for stuck actuators, a fixed value in the output's place.  ``BatchedAOEnv(servo=dict(...))`` puts one between
``step(actions)`` and the mirror; ``info["applied_action"]`` is what the mirror received.  The loop delay a controller sees is then
``1 + latency`` frames (the one frame of measure-then-act plus the servo's): pass that to ``telemetry.gain_limit``, ``default_grid`` and
``ModalIntegrator(delay=...)``.

The history from before an env's last reset is the rest command 0.  On an env whose action is the actuators (``SH_operation=True``: every
controller of ``rollout``) that is the flat mirror.  An env with the reference's normalised action chain divides the action by the rms of
the surface it makes, so an all-zero action is 0 / 0 there, with or without a servo: for the first ``ceil(latency)`` frames of an episode
such an env returns NaN outputs, exactly what its servo-less twin returns for a zero action.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .device_handle import DeviceHandle, ptr
from .params import resolve_per_env

MAX_LATENCY, MAX_ACT = _lib.SERVO_MAX_LATENCY, _lib.SERVO_MAX_ACT


def resolve_stuck(stuck, num_envs, act_dim):
    """``stuck`` as (mask [B, A] uint8, value [B, A] float32): None (no dead actuator), ``{actuator index: value}`` (every env), or a pair
    ``(mask, value)`` of [A] or [B, A] arrays.  ``ValueError`` for an index outside the mirror, wrong shapes and non-finite values."""
    B, A = int(num_envs), int(act_dim)
    mask, value = np.zeros((B, A), dtype=np.uint8), np.zeros((B, A), dtype=np.float32)
    if stuck is None:
        return mask, value
    if isinstance(stuck, dict):
        for j, v in stuck.items():
            if isinstance(j, bool) or int(j) != j or not 0 <= int(j) < A:
                raise ValueError(f"stuck: actuator {j!r} is not one of the mirror's {A}")
            if not abs(float(v)) <= float(np.finfo(np.float32).max):   # (NaN included)
                raise ValueError(f"stuck: the value of actuator {j!r} must be finite (got {v!r})")
            mask[:, int(j)] = 1
            value[:, int(j)] = float(v)
        return mask, value
    if not isinstance(stuck, (tuple, list)) or len(stuck) != 2:
        raise ValueError("stuck: None, a dict {actuator index: value} or a pair (mask, value) of [A] or [B, A] arrays")
    m, v = np.asarray(stuck[0]), np.asarray(stuck[1], dtype=np.float64)
    if m.shape not in ((A,), (B, A)) or v.shape not in ((A,), (B, A)) or m.dtype.kind not in "bui":
        raise ValueError(f"stuck: the mask (bool) and the values are [{A}] or [{B}, {A}] arrays (got shapes {m.shape} and {v.shape})")
    mask[:] = m != 0
    with np.errstate(over="ignore"):
        value[:] = np.where(mask != 0, np.broadcast_to(v, (B, A)), 0.0).astype(np.float32)
    if not np.all(np.isfinite(value)):
        raise ValueError("stuck: the value of every stuck actuator must be finite in float32")
    return mask, value


def resolve_servo(num_envs, total_envs, global_env_offset, act_dim, latency=0.0, response=1.0, stroke=None, stuck=None, max_latency=None):
    """The servo's arguments, checked: dict(latency, response, stroke [B] float64; stuck [B, A] uint8; stuck_value [B, A] float32;
    max_latency int).  ``latency``, ``response`` and ``stroke`` are scalars or per-env values under ``params.resolve_per_env``'s rules
    (``stroke`` None or +inf: no limit).  ``ValueError`` for act_dim outside 1 .. 128, latency < 0 or above ``max_latency`` (0 .. 4; default
    ceil of the largest latency), response outside (0, 1], stroke <= 0."""
    B, A = int(num_envs), int(act_dim)
    if not 1 <= A <= MAX_ACT:
        raise ValueError(f"servo: act_dim must lie in 1 .. {MAX_ACT} (got {act_dim!r})")
    lat = resolve_per_env("latency", latency, B, total_envs, global_env_offset)[0]
    resp = resolve_per_env("response", response, B, total_envs, global_env_offset)[0]
    if stroke is None:
        limit = np.full(B, np.inf)
    else:
        # (+inf means no limit; resolve_per_env takes finite values, so the limits and the places of the infinities go through it apart)
        s = np.asarray(stroke, dtype=np.float64)
        limit = resolve_per_env("stroke", np.where(np.isposinf(s), 1.0, s), B, total_envs, global_env_offset)[0]
        free = resolve_per_env("stroke", np.isposinf(s).astype(np.float64), B, total_envs, global_env_offset)[0]
        limit = np.where(free > 0, np.inf, limit)
    if np.any(lat < 0):
        raise ValueError(f"latency must be >= 0 frames (got {latency!r})")
    if np.any(resp <= 0) or np.any(resp > 1):
        raise ValueError(f"response must lie in (0, 1] (got {response!r})")
    if np.any(limit <= 0):
        raise ValueError(f"stroke must be > 0 (got {stroke!r})")
    if max_latency is None:
        max_latency = int(math.ceil(float(lat.max())))
    if isinstance(max_latency, bool) or int(max_latency) != max_latency or not 0 <= int(max_latency) <= MAX_LATENCY:
        raise ValueError(f"max_latency must be an integer in 0 .. {MAX_LATENCY} frames (got {max_latency!r}; the largest latency asked for is {lat.max()})")
    if lat.max() > int(max_latency):
        raise ValueError(f"latency {lat.max()} exceeds max_latency = {int(max_latency)}")
    mask, value = resolve_stuck(stuck, B, A)
    return dict(latency=lat, response=resp, stroke=limit, stuck=mask, stuck_value=value, max_latency=int(max_latency))


class MirrorServo(DeviceHandle):
    """The servo of ``env`` (any ``BatchedAOEnv``, for its batch, action width, global env ids and device).

    latency      frames between a command and the mirror's drive, >= 0, fractional allowed: at call n the drive is the command of call
                 n - latency, linearly interpolated between the two nearest calls.
    response     in (0, 1]: the share of the way to its drive the mirror moves per frame (1: it is there at once).
    stroke       None (no limit) or > 0: the drive is clipped to [-stroke, stroke], in the action's own unit.
    stuck        None, ``{actuator index: value}`` or ``(mask, value)`` arrays [A] or [B, A]: those actuators sit at ``value``.
    max_latency  whole frames the history holds, 0 .. 4 (default: ceil of the largest latency); ``set_params`` can move ``latency`` up to it.

    ``latency``, ``response`` and ``stroke`` are scalars or per-env values (``num_envs`` values, or ``total_envs`` values indexed by the
    global env id).  ``apply(actions, mask=None, out=None)`` pushes one frame's [B, A] float32 command and returns what the mirror receives
    (rows of envs the mask leaves out are not written, and those envs keep their state); ``reset(mask=None)`` puts the selected envs'
    history and mirror to rest (0); ``set_params(...)`` replaces the named arguments; ``state_dict()`` / ``load_state_dict()`` resume
    bit-identically.  Everything runs on the caller's current stream; the arithmetic is float64, one rounded operation at a time
    (``include/aogym_servo.h``), so ``tests/servo_reference.py`` replays it bit for bit and servos over the parts of a batch reproduce the
    whole.  With the defaults ``apply`` returns the bits of its input."""

    prefix, noun = "aog_servo", "servo"

    def __init__(self, env, latency=0.0, response=1.0, stroke=None, stuck=None, max_latency=None):
        import torch

        self.num_envs, self.act_dim = int(env.num_envs), int(env.num_modes)
        self.total_envs, self.global_env_offset = int(env.total_envs), int(env.global_env_offset)
        self._given = dict(latency=latency, response=response, stroke=stroke, stuck=stuck)
        plan = resolve_servo(self.num_envs, self.total_envs, self.global_env_offset, self.act_dim, max_latency=max_latency, **self._given)
        self.max_latency = plan.pop("max_latency")
        self.params = plan
        self._bind(torch, env.device, self.num_envs)
        self._create()
        self._push()

    def _config(self):
        return _lib.AogServoConfig(_lib.ABI_VERSION, self.num_envs, self.act_dim, self.max_latency)

    def _push(self):
        host = [np.ascontiguousarray(self.params[k]) for k in ("latency", "response", "stroke", "stuck", "stuck_value")]
        self._call("set_params", *[h.ctypes.data_as(C.c_void_p) for h in host])

    def set_params(self, **changed):
        """Replace ``latency``, ``response``, ``stroke`` and / or ``stuck`` (the constructor's forms; ``latency`` up to ``max_latency``);
        the state stays.  The copy is blocking but not ordered behind this stream's pending calls, so the stream is synchronised first."""
        unknown = set(changed) - set(self._given)
        if unknown:
            raise ValueError(f"set_params: unknown arguments {sorted(unknown)} (latency, response, stroke, stuck)")
        given = {**self._given, **changed}
        plan = resolve_servo(self.num_envs, self.total_envs, self.global_env_offset, self.act_dim, max_latency=self.max_latency, **given)
        plan.pop("max_latency")
        self._torch.cuda.current_stream(self.device).synchronize()
        self._given, self.params = given, plan
        self._push()

    def reset(self, mask=None):
        """History and mirror of the selected envs (all without a mask) to rest: every command from before reads as 0."""
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    def apply(self, actions, mask=None, out=None):
        """One frame: ``actions`` [B, A] float32 (contiguous, on the device) is the command; returns the [B, A] float32 action the mirror
        receives (``out``, or a new tensor; rows of envs the mask leaves out are not written — zeros in a new tensor)."""
        torch = self._torch
        shape = (self.num_envs, self.act_dim)
        a = self._tensor(actions, shape, torch.float32, f"apply: actions must be a contiguous float32 {list(shape)} tensor on {self.device}")
        m = self._mask(mask, "apply")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device) if m is None else torch.zeros(shape, dtype=torch.float32, device=self.device)
        else:
            self._tensor(out, shape, torch.float32, f"apply: out must be a contiguous float32 {list(shape)} tensor on {self.device}")
        self._call("apply", ptr(a), ptr(m), ptr(out), self._stream())
        return out

    def state_dict(self):
        return {"blob": self.get_state(), "num_envs": self.num_envs, "act_dim": self.act_dim, "max_latency": self.max_latency}

    def check_state_dict(self, state):
        """``ValueError`` unless ``state`` is the ``state_dict()`` of a servo of this configuration; nothing is touched."""
        if any(int(state.get(k, -1)) != getattr(self, k) for k in ("num_envs", "act_dim", "max_latency")):
            raise ValueError(f"load_state_dict: the state is of another servo (this one: {self.num_envs} envs, {self.act_dim} actuators, "
                             f"max_latency {self.max_latency})")

    def load_state_dict(self, state):
        self.check_state_dict(state)
        self.set_state(state["blob"])
