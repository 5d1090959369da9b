"""Sensorless adaptive optics: stochastic parallel gradient descent (SPGD) on the device.

The environment is a wavefront-sensorless problem: the agent sees a tiny focal-plane observation and a scalar quality.  Every other
classical controller of ``rollout`` (``'shack'``, ``'ideal'``, ``'pyramid'``, ``'predictive'``, ``'modal'``) reads a wavefront sensor or
the true wavefront; SPGD, the standard method of free-space optical links, uses only that scalar, so it is the classical baseline with the
information a learnt policy has.  ``SPGDController`` runs two-sided SPGD with Bernoulli perturbations per env (``aog_spgd_*``,
``csrc/k_spgd.h``): it applies ``u + amplitude delta``, then ``u - amplitude delta``, and moves ``u`` by
``gain (J_plus - J_minus) delta``; one iteration takes two env steps.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib
from .device_handle import DeviceHandle, ptr

METRICS = ("power", "strehl", "reward")


def _per_env(name, value, num_envs):
    """``value`` (a scalar or ``num_envs`` values) as a float64 array [num_envs] of finite, non-negative numbers; ValueError otherwise."""
    import numpy as np

    v = np.asarray(value, dtype=np.float64)
    if v.ndim == 0:
        v = np.full((num_envs,), float(v))
    if v.shape != (num_envs,):
        raise ValueError(f"{name}: expected a scalar or {num_envs} values, got shape {v.shape}")
    if not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError(f"{name} must be finite and >= 0 (got {value!r})")
    return np.ascontiguousarray(v)


class SPGDController(DeviceHandle):
    """SPGD for an env built with ``SH_operation=True`` (``BatchedAOEnv`` or ``LayeredAOEnv``), whose action is the raw actuator vector.

    ``gain`` and ``amplitude`` are scalars or per-env values (a batch can sweep them); ``metric`` names the step output it climbs
    (``"power"``: fibre-coupled power, ``"strehl"``, ``"reward"``) — the float32 the step stores; ``clip`` bounds ``|u_i|`` (0: no bound);
    ``seed`` keys the perturbation streams (default: the env's), which are Philox4x32-10 streams of the GLOBAL env id, so a split batch
    reproduces the whole one.

    ``reset(mask)`` starts the masked envs (all without a mask) from a flat command — or from the env's actuators when it was built with
    ``flat_mirror_start_per_episode=False`` — keeps their iteration counters and returns the first command.  ``action()`` is one query on
    the metric of the env's last step, ``update(metric)`` the same on a caller's own float32 ``[B]`` tensor; both return the next command,
    ``[B, A]`` float32.  ``env.reset_with_spgd(ctrl)`` / ``env.step_with_spgd(ctrl)`` run the same query inside the step's last launch.
    ``centre()`` is ``u``; ``get_state`` / ``set_state`` resume bit-identically (the state blob holds per env u [A] and J_plus float64, then
    k and h uint32)."""

    prefix, noun = "aog_spgd", "controller"

    def __init__(self, env, gain=1.0, amplitude=0.05, metric="power", clip=0.0, seed=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS} (got {metric!r})")
        if not getattr(env, "SH_operation", False):
            raise ValueError("SPGDController needs an env created with SH_operation=True: otherwise the action is rescaled to a fixed surface rms "
                             "and a perturbation amplitude means nothing")
        B, A = int(env.num_envs), int(env.num_modes)
        gain, amplitude = _per_env("gain", gain, B), _per_env("amplitude", amplitude, B)
        clip = float(clip)
        if not math.isfinite(clip) or clip < 0:
            raise ValueError(f"clip must be finite and >= 0 (got {clip})")
        self.env = env
        self.metric = metric
        self.clip = clip
        self.seed = int(env._base_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.num_envs, self.act_dim = B, A
        self.env_id_base = int(getattr(env, "global_env_offset", 0))
        self._bind(env._torch, env.device, B)
        self._create()
        self.set_params(gain, amplitude)

    def _config(self):
        return _lib.AogSpgdConfig(_lib.ABI_VERSION, self.num_envs, self.act_dim, self.env_id_base, self.seed, _lib.AOG_SPGD_METRIC[self.metric], 0, self.clip)

    def _out(self, out, masked, who):
        torch = self._torch
        if out is None:
            return (torch.zeros if masked else torch.empty)((self.num_envs, self.act_dim), dtype=torch.float32, device=self.device)
        return self._tensor(out, (self.num_envs, self.act_dim), torch.float32,
                            f"{who}: out must be a contiguous float32 [{self.num_envs}, {self.act_dim}] tensor on {self.device}")

    def set_params(self, gain=None, amplitude=None):
        """New per-env ``gain`` / ``amplitude`` (scalars or ``[B]`` values; None keeps the current ones)."""
        gain = self.gain if gain is None else _per_env("gain", gain, self.num_envs)
        amplitude = self.amplitude if amplitude is None else _per_env("amplitude", amplitude, self.num_envs)
        self._torch.cuda.current_stream(self.device).synchronize()   # (the copy is blocking but not ordered behind this stream's queries)
        self._call("set_params", gain.ctypes.data_as(C.c_void_p), amplitude.ctypes.data_as(C.c_void_p))
        self.gain, self.amplitude = gain, amplitude

    def reset(self, mask=None, out=None):
        """Reset the masked envs (all without a mask) and return the command ``u + amplitude delta_k`` (rows of other envs: untouched,
        zeros in a fresh tensor)."""
        m = self._mask(mask, "reset")
        out = self._out(out, m is not None, "reset")
        start = None if self.env.flat_mirror_start_per_episode else self.env.get_actuators()
        self._call("reset", ptr(m), ptr(start), ptr(out), self._stream())
        return out

    def update(self, metric, mask=None, out=None):
        """One query on ``metric`` (float32 ``[B]`` device tensor): the next command."""
        self._tensor(metric, (self.num_envs,), self._torch.float32, f"update: metric must be a contiguous float32 [{self.num_envs}] tensor on {self.device}")
        m = self._mask(mask, "update")
        out = self._out(out, m is not None, "update")
        self._call("update", ptr(metric), ptr(m), ptr(out), self._stream())
        return out

    def action(self, out=None):
        """One query on the metric the env's last ``step`` stored."""
        last = getattr(self.env, "_last_step", None)
        if last is None:
            raise ValueError("SPGDController.action: the env has not stepped since its last reset (reset() gives the first command)")
        return self.update(self.step_metric(last), out=out)

    def step_metric(self, step_ret):
        """The tensor of a step tuple this controller descends on."""
        return step_ret[1] if self.metric == "reward" else step_ret[4][self.metric]

    def unpack(self, blob=None):
        """A blob as a dict of tensors: u [B, A] float64, J_plus [B] float64, k [B] and h [B] int64 (copies)."""
        torch = self._torch
        blob = self.get_state() if blob is None else blob
        B, A = self.num_envs, self.act_dim
        words = blob.view(torch.float64).reshape(B, A + 2)
        kh = blob.view(torch.int32).reshape(B, 2 * (A + 2))[:, -2:].to(torch.int64) & 0xFFFFFFFF
        return {"u": words[:, :A].clone(), "J_plus": words[:, A].clone(), "k": kh[:, 0].clone(), "h": kh[:, 1].clone()}

    def centre(self):
        """The centre command u, [B, A] float64."""
        return self.unpack()["u"]
