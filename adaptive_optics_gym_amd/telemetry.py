"""Closed-loop modal telemetry: what the loop measured over time, and the classical baseline it yields.

``ModalTelemetry`` records per-env pseudo-open-loop (POL) measurements — the actuator vectors that would have flattened the wavefront at the
steps they were taken — in a ring on the device (``aog_telemetry_*``, ``csrc/k_telemetry.h``), returns Welch's temporal power spectral
density of every mode, and from it the integrator gain per mode that minimises the residual the density predicts given the loop delay
(Gendron and Léna's optimised modal gains): a slow, noisy high-order mode gets a low gain, a fast, bright low-order mode a high one.
``ModalIntegrator`` is the integrator that runs those gains, the baseline every learnt controller is reported against
(``rollout(policy="modal", controller=...)``).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib
from .device_handle import DeviceHandle, check_measurement, ptr

MAX_MODES, MIN_LENGTH, MAX_LENGTH, MIN_SEGMENT, MAX_GRID, MAX_DELAY = 128, 64, 1024, 32, 64, 4


def gain_limit(delay):
    """The largest stable gain of the integrator a <- a + g m with ``delay`` frames of lag: 2 sin(pi / (2 (2 d - 1))), where a root of
    z^d - z^(d-1) + g reaches the unit circle (2 at d = 1, 1 at d = 2)."""
    d = int(delay)
    if d != delay or d < 1 or d > MAX_DELAY:
        raise ValueError(f"delay must be 1, 2, 3 or 4 (got {delay!r})")
    return 2.0 * math.sin(math.pi / (2.0 * (2 * d - 1)))


def default_grid(delay=1):
    """32 candidates log-spaced from 0.02 to 0.8 of ``gain_limit(delay)``."""
    import numpy as np

    g = gain_limit(delay)
    return np.geomspace(0.02 * g, 0.8 * g, 32)


def _is_pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def check_segment(segment, length):
    s = int(segment)
    if s != segment or not _is_pow2(s) or s < MIN_SEGMENT or s > length:
        raise ValueError(f"segment must be a power of two in [{MIN_SEGMENT}, length {length}] (got {segment!r})")
    return s


def check_grid(grid, delay):
    """The candidates as a contiguous float64 array: at most 64, ascending, each inside (0, gain_limit(delay))."""
    import numpy as np

    g_max = gain_limit(delay)
    g = np.ascontiguousarray(default_grid(delay) if grid is None else grid, dtype=np.float64)
    if g.ndim != 1 or not 1 <= g.size <= MAX_GRID:
        raise ValueError(f"grid must be a vector of 1 to {MAX_GRID} gains (got shape {g.shape})")
    if not np.all((g > 0.0) & (g < g_max)):
        raise ValueError(f"grid: every gain must lie in (0, {g_max}), the stable gains at delay {delay} (got {g.min()} .. {g.max()})")
    if np.any(np.diff(g) <= 0.0):
        raise ValueError("grid must be strictly ascending")
    return g


class ModalTelemetry(DeviceHandle):
    """``num_envs`` rings of ``length`` measurements of ``act_dim`` modes, float64 on ``device`` (the library handle ``aog_telemetry``; it is
    made on first use).  ``push(y, mask=None)`` stores one row per selected env (a row with a non-finite value is skipped and counted);
    ``psd(segment=None)`` -> (freq_bins [S/2+1] in cycles per frame, psd [B, A, S/2+1], segments [B] int32): Welch's estimate, periodic Hann
    window, hop S/2, the variance per bin; NaN rows and 0 segments while an env holds fewer than S samples.
    ``optimise_gains(delay=1, grid=None, segment=None, with_costs=False)`` -> (gain [B, A], cost [B, A][, cost_all [B, A, G]]): per mode the
    first candidate of ``grid`` (default ``default_grid(delay)``) that minimises J(g) = sum_k |R_k(g)|^2 Phi[k].  ``segment`` defaults to
    ``length // 4`` (32 at length 64).  Rows of envs a ``mask`` leaves out are NaN (0 segments) in fresh outputs.  ``state_dict`` / ``load_state_dict``
    resume bit-identically; a batch split over several instances reproduces the whole one bit for bit.  The state blob of ``get_state`` /
    ``set_state`` holds per env hist [T, A] float64, count and skipped int64."""

    prefix, noun, lazy = "aog_telemetry", "telemetry", True

    def __init__(self, num_envs, act_dim, length=512, device=None, global_env_offset=0):
        import torch

        self.num_envs, self.act_dim, self.length = int(num_envs), int(act_dim), int(length)
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1 (got {num_envs})")
        if not 1 <= self.act_dim <= MAX_MODES:
            raise ValueError(f"act_dim must lie in [1, {MAX_MODES}] (got {act_dim})")
        if not _is_pow2(self.length) or not MIN_LENGTH <= self.length <= MAX_LENGTH:
            raise ValueError(f"length must be a power of two in [{MIN_LENGTH}, {MAX_LENGTH}] (got {length})")
        self.global_env_offset = int(global_env_offset)
        self._bind(torch, device, self.num_envs)
        self.default_segment = max(MIN_SEGMENT, self.length // 4)

    def _config(self):
        return _lib.AogTelemetryConfig(self.num_envs, self.act_dim, self.length, self.global_env_offset)

    def _out(self, shape, m, dtype=None):
        torch = self._torch
        dtype = dtype or torch.float64
        if m is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return torch.full(shape, float("nan") if dtype == torch.float64 else 0, dtype=dtype, device=self.device)

    # -- the calls
    def push(self, y, mask=None):
        self._tensor(y, (self.num_envs, self.act_dim), self._torch.float64,
                     f"push: y must be a contiguous float64 [{self.num_envs}, {self.act_dim}] tensor on {self.device}")
        self._call("push", ptr(y), ptr(self._mask(mask, "push")), self._stream())

    def psd(self, segment=None, mask=None):
        torch = self._torch
        S = check_segment(self.default_segment if segment is None else segment, self.length)
        m = self._mask(mask, "psd")
        psd = self._out((self.num_envs, self.act_dim, S // 2 + 1), m)
        seg = self._out((self.num_envs,), m, torch.int32)
        self._call("psd", S, ptr(psd), ptr(seg), ptr(m), self._stream())
        freq = torch.arange(S // 2 + 1, dtype=torch.float64, device=self.device) / S
        return freq, psd, seg

    def optimise_gains(self, delay=1, grid=None, segment=None, with_costs=False, mask=None):
        S = check_segment(self.default_segment if segment is None else segment, self.length)
        g = check_grid(grid, delay)
        m = self._mask(mask, "optimise_gains")
        B, A = self.num_envs, self.act_dim
        gain, cost = self._out((B, A), m), self._out((B, A), m)
        cost_all = self._out((B, A, g.size), m) if with_costs else None
        self._call("gains", S, int(delay), g.ctypes.data_as(C.POINTER(C.c_double)), int(g.size), ptr(gain), ptr(cost), ptr(cost_all), ptr(m),
                   self._stream())
        return (gain, cost, cost_all) if with_costs else (gain, cost)

    def reset(self, mask=None):
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    def state_bytes(self):
        return 8 * self.num_envs * (self.length * self.act_dim + 2)

    _state_bytes = state_bytes   # (no handle needed)

    def unpack(self, blob=None):
        """A blob as a dict of tensors: hist [B, T, A] float64, count [B], skipped [B] int64 (copies)."""
        torch = self._torch
        blob = self.get_state() if blob is None else blob
        B, T, A = self.num_envs, self.length, self.act_dim
        words = blob.view(torch.float64).reshape(B, T * A + 2)
        ints = blob.view(torch.int64).reshape(B, T * A + 2)
        return {"hist": words[:, :T * A].reshape(B, T, A).clone(), "count": ints[:, -2].clone(), "skipped": ints[:, -1].clone()}

    def state_dict(self):
        return {"blob": self.get_state(), "num_envs": self.num_envs, "act_dim": self.act_dim, "length": self.length}

    def load_state_dict(self, state):
        for k in ("num_envs", "act_dim", "length"):
            if state[k] != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]}, this telemetry has {getattr(self, k)}")
        self.set_state(state["blob"])


class ModalIntegrator:
    """The modal integrator of an env (``BatchedAOEnv`` or ``LayeredAOEnv``) with one gain per (env, mode): ``gains`` [B, A] float64 on the
    device, ``gain`` everywhere until ``retune()``.

    ``action()`` takes the pseudo-open-loop measurement y exactly as ``PredictiveController`` does (``measurement="truth"``:
    ``env.ideal_action()``; ``"pyramid"``: the pyramid integrator at gain 1), and returns ``update(y)``: y goes into ``telemetry``
    (a ``ModalTelemetry``, made here unless one is passed), the residual measurement is m = y - a with a the command this integrator last
    returned, and a <- leak a + gains * m — [B, A] float64 actuators in the form ``ideal_action()`` returns.  A row of y with a
    non-finite value leaves its env's command as it was.  ``retune(grid=None, segment=None)`` sets ``gains`` to
    ``telemetry.optimise_gains(delay, grid, segment)`` (envs that hold fewer samples than a segment keep theirs) and returns the
    predicted costs.  ``delay`` is the lag, in frames, between a measurement and the command it yields reaching the mirror: 1 in
    ``rollout``'s loop, and ``1 + latency`` for an env built with ``servo=dict(latency=...)`` (``servo.MirrorServo``: whole frames here; round
    a fractional latency up, the conservative side of ``gain_limit``)."""

    def __init__(self, env, measurement="truth", delay=1, gain=0.4, leak=1.0, telemetry=None):
        check_measurement(env, measurement)
        g_max = gain_limit(delay)
        gain, leak = float(gain), float(leak)
        if not 0.0 < gain < g_max:
            raise ValueError(f"gain must lie in (0, {g_max}), the stable gains at delay {delay} (got {gain})")
        if not 0.0 < leak <= 1.0:
            raise ValueError(f"leak must lie in (0, 1] (got {leak})")
        B, A = int(env.num_envs), int(env.num_modes)
        if telemetry is None:
            telemetry = ModalTelemetry(B, A, device=env.device, global_env_offset=int(getattr(env, "global_env_offset", 0)))
        elif (telemetry.num_envs, telemetry.act_dim) != (B, A):
            raise ValueError(f"telemetry holds [{telemetry.num_envs}, {telemetry.act_dim}] measurements, the env gives [{B}, {A}]")
        import torch

        self.env, self.measurement, self.delay, self.leak, self.telemetry = env, measurement, int(delay), leak, telemetry
        self.gains = torch.full((B, A), gain, dtype=torch.float64, device=telemetry.device)
        self.command = torch.zeros((B, A), dtype=torch.float64, device=telemetry.device)
        self.measurement_value = None

    def action(self):
        from .predictor import pseudo_open_loop

        return self.update(pseudo_open_loop(self.env, self.measurement, "ModalIntegrator.action"))

    def update(self, y, mask=None):
        import torch

        self.telemetry.push(y, mask)
        keep = torch.isfinite(y).all(dim=1, keepdim=True)
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=y.device).to(torch.bool)[:, None]
        a = self.command
        self.command = torch.where(keep, self.leak * a + self.gains * (y - a), a)
        self.measurement_value = y
        return self.command

    def retune(self, grid=None, segment=None):
        import torch

        gain, cost = self.telemetry.optimise_gains(self.delay, grid, segment)
        self.gains = torch.where(torch.isnan(gain), self.gains, gain)
        return cost

    def reset(self, mask=None):
        """The selected envs' commands back to zero and their telemetry emptied (the gains stay)."""
        import torch

        self.telemetry.reset(mask)
        if mask is None:
            self.command = torch.zeros_like(self.command)
        else:
            self.command = torch.where(torch.as_tensor(mask, device=self.command.device).to(torch.bool)[:, None], torch.zeros_like(self.command), self.command)

    def state_dict(self):
        return {"telemetry": self.telemetry.state_dict(), "gains": self.gains.clone(), "command": self.command.clone(), "delay": self.delay,
                "leak": self.leak}

    def load_state_dict(self, state):
        for k in ("delay", "leak"):
            if state[k] != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]}, this integrator has {getattr(self, k)}")
        self.telemetry.load_state_dict(state["telemetry"])
        self.gains = state["gains"].to(self.gains.device).clone()
        self.command = state["command"].to(self.command.device).clone()

    def close(self):
        self.telemetry.close()
