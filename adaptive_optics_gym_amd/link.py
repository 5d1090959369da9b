"""Link telemetry: the read-out of the free-space optical link next to the astronomer's Strehl.

``LinkTelemetry`` records the fibre-coupled power of every env (``info["power"]`` of a step) in a ring on the device (``aog_link_*``,
``csrc/k_link.h``) and returns, over what the ring holds, the figures a link engineer judges a controller by: how often the power drops
below a threshold, how many fades there were and how long they lasted, the scintillation index, the power histogram and the mean
bit-error rate of on-off keying.  Nothing is copied to the host; ``rollout(..., link=LinkTelemetry(...))`` feeds it.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib
from .device_handle import DeviceHandle, ptr

MIN_LENGTH, MAX_LENGTH, MAX_THRESHOLDS, MAX_HIST_EDGES, MAX_Q = 64, 4096, 16, 64, 8


def default_hist_edges_db():
    """32 edges evenly spaced in dB from -30 to +6."""
    import numpy as np

    return np.linspace(-30.0, 6.0, 32)


def db_to_factor(db):
    """dB relative to the reference level as the linear factors 10^(dB / 10) the library takes (float64)."""
    import numpy as np

    return np.power(10.0, np.asarray(db, dtype=np.float64) / 10.0)


def check_db(name, db, limit):
    """``db`` as a contiguous float64 vector of at most ``limit`` finite, strictly ascending values."""
    import numpy as np

    v = np.ascontiguousarray(db, dtype=np.float64)
    if v.ndim != 1 or v.size > limit:
        raise ValueError(f"{name} must be a vector of at most {limit} values in dB (got shape {v.shape})")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{name}: every value must be finite")
    if np.any(np.diff(v) <= 0.0):
        raise ValueError(f"{name} must be strictly ascending")
    return v


def check_q(q):
    """The receiver Q factors as a contiguous float64 vector of at most 8 positive finite values."""
    import numpy as np

    v = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if v.size > MAX_Q:
        raise ValueError(f"q must hold at most {MAX_Q} Q factors (got {v.size})")
    if not np.all(np.isfinite(v) & (v > 0.0)):
        raise ValueError("q: every Q factor must be positive and finite")
    return v


def check_reference(reference):
    """``reference`` as (mode, value): ``"mean"`` (each env's own mean power) or a positive finite absolute level."""
    if isinstance(reference, str):
        if reference != "mean":
            raise ValueError(f"reference must be 'mean' or a positive power (got {reference!r})")
        return _lib.AOG_LINK_REF["mean"], 0.0
    r = float(reference)
    if not math.isfinite(r) or r <= 0.0:
        raise ValueError(f"reference must be 'mean' or a positive finite power (got {reference!r})")
    return _lib.AOG_LINK_REF["absolute"], r


class LinkTelemetry(DeviceHandle):
    """``num_envs`` rings of ``length`` float32 power samples on ``device`` (the library handle ``aog_link``; it is made on first use).
    ``push(power, mask=None)`` stores one sample per selected env (a non-finite one is skipped and counted).
    ``statistics(thresholds_db=(-10, -6, -3), reference="mean", hist_edges_db=None, q=(), mask=None)`` -> a dict of device tensors over each
    env's window, the last n = min(count, length) samples: ``samples`` [B] int32 (n), ``mean``, ``mean_square``, ``scintillation_index``
    (mean_square / mean^2 - 1), ``reference`` (the level P thresholds, edges and BER refer to: the env's own mean, or the absolute power
    passed as ``reference``) [B] float64, ``minimum``, ``maximum`` [B] float32; per threshold (dB relative to P) ``below`` (samples in fade),
    ``fade_fraction`` (below / n), ``fades`` (maximal runs of consecutive in-fade samples), ``mean_fade_duration`` (below / fades in frames,
    NaN without a fade) and ``longest_fade`` [B, K]; ``hist`` [B, E + 1] int32 over the E ``hist_edges_db`` (default: 32 edges from -30 to
    +6 dB; bin 0 below the first edge, bin E from the last edge up) with ``hist_edges`` [B, E] float64, the edges in units of power; ``ber``
    [B, Q] float64, the mean of erfc(q p / (P sqrt 2)) / 2 (on-off keying at receiver Q factor q at the reference level).  An empty window
    gives 0 in the integer fields and NaN in the float ones, and so do the rows of envs a ``mask`` leaves out.  One kernel launch; the derived
    fields are torch arithmetic on its outputs.  ``state_dict`` / ``load_state_dict`` resume bit-identically; a batch split over several
    instances reproduces the whole one bit for bit.  The state blob of ``get_state`` / ``set_state`` holds per env ring [T] float32, count and
    skipped int64."""

    prefix, noun, lazy = "aog_link", "link telemetry", True

    def __init__(self, num_envs, length=1024, device=None, global_env_offset=0):
        import torch

        self.num_envs, self.length = int(num_envs), int(length)
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1 (got {num_envs})")
        if self.length & (self.length - 1) or not MIN_LENGTH <= self.length <= MAX_LENGTH:
            raise ValueError(f"length must be a power of two in [{MIN_LENGTH}, {MAX_LENGTH}] (got {length})")
        self.global_env_offset = int(global_env_offset)
        self._bind(torch, device, self.num_envs)

    def _config(self):
        return _lib.AogLinkConfig(_lib.ABI_VERSION, self.num_envs, self.length, self.global_env_offset, 0)

    def _out(self, shape, m, dtype):   # (fresh outputs: rows a mask leaves out read NaN / 0)
        torch = self._torch
        if m is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return torch.full(shape, 0 if dtype == torch.int32 else float("nan"), dtype=dtype, device=self.device)

    # -- the calls
    def push(self, power, mask=None):
        self._tensor(power, (self.num_envs,), self._torch.float32, f"push: power must be a contiguous float32 [{self.num_envs}] tensor on {self.device}")
        self._call("push", ptr(power), ptr(self._mask(mask, "push")), self._stream())

    def statistics(self, thresholds_db=(-10.0, -6.0, -3.0), reference="mean", hist_edges_db=None, q=(), mask=None):
        torch = self._torch
        th_db = check_db("thresholds_db", thresholds_db, MAX_THRESHOLDS)
        he_db = check_db("hist_edges_db", default_hist_edges_db() if hist_edges_db is None else hist_edges_db, MAX_HIST_EDGES)
        qs = check_q(q)
        mode, level = check_reference(reference)
        m = self._mask(mask, "statistics")
        f, g = db_to_factor(th_db), db_to_factor(he_db)
        B, K, E, Q = self.num_envs, f.size, g.size, qs.size
        i32, f32, f64 = torch.int32, torch.float32, torch.float64
        samples, mean, msq = self._out((B,), m, i32), self._out((B,), m, f64), self._out((B,), m, f64)
        mn, mx, ref = self._out((B,), m, f32), self._out((B,), m, f32), self._out((B,), m, f64)
        below, fades, longest = (self._out((B, K), m, i32) for _ in range(3))
        hist, ber = self._out((B, E + 1), m, i32), self._out((B, Q), m, f64)

        def host(a):
            return a.ctypes.data_as(C.POINTER(C.c_double))

        self._call("statistics", mode, level, host(f), K, host(g), E, host(qs), Q, ptr(samples), ptr(mean), ptr(msq), ptr(mn), ptr(mx), ptr(ref),
                   ptr(below), ptr(fades), ptr(longest), ptr(hist), ptr(ber), ptr(m), self._stream())
        nan = torch.full((), float("nan"), dtype=f64, device=self.device)
        n = samples.to(f64).unsqueeze(1)
        return {"samples": samples, "mean": mean, "mean_square": msq, "scintillation_index": msq / (mean * mean) - 1.0, "minimum": mn, "maximum": mx,
                "reference": ref, "below": below, "fade_fraction": torch.where(n > 0, below / n, nan), "fades": fades,
                "mean_fade_duration": torch.where(fades > 0, below / fades.to(f64), nan), "longest_fade": longest, "hist": hist,
                "hist_edges": ref.unsqueeze(1) * torch.as_tensor(g, device=self.device), "ber": ber}

    def reset(self, mask=None):
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    def state_bytes(self):
        return self.num_envs * (4 * self.length + 16)

    _state_bytes = state_bytes   # (no handle needed)

    def unpack(self, blob=None):
        """A blob as a dict of tensors: ring [B, T] float32 (sample c at c mod T), count [B], skipped [B] int64 (copies)."""
        torch = self._torch
        blob = self.get_state() if blob is None else blob
        B, T = self.num_envs, self.length
        rec = blob.reshape(B, 4 * T + 16)
        ints = rec[:, 4 * T:].contiguous().view(torch.int64)
        return {"ring": rec[:, :4 * T].contiguous().view(torch.float32), "count": ints[:, 0].clone(), "skipped": ints[:, 1].clone()}

    def window(self, blob=None):
        """The chronological windows as a list of B float32 tensors (oldest first), from a blob or the current state (one host copy of the counts)."""
        u = self.unpack(blob)
        out = []
        for ring, count in zip(u["ring"], u["count"].tolist()):
            n = max(0, min(count, self.length))
            out.append(ring[:n].clone() if count <= self.length else self._torch.roll(ring, -(count % self.length)))
        return out

    def state_dict(self):
        return {"blob": self.get_state(), "num_envs": self.num_envs, "length": self.length}

    def load_state_dict(self, state):
        for k in ("num_envs", "length"):
            if state[k] != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]}, this link telemetry has {getattr(self, k)}")
        self.set_state(state["blob"])


def check_link(link, env):
    """ValueError unless ``link`` is a ``LinkTelemetry`` built for ``env``'s num_envs and device (``rollout(..., link=)``)."""
    import torch

    if not isinstance(link, LinkTelemetry):
        raise ValueError(f"link must be a LinkTelemetry (got {type(link).__name__})")
    if link.num_envs != int(env.num_envs):
        raise ValueError(f"link holds {link.num_envs} envs, the env has {env.num_envs}")
    dev = torch.device(env.device)
    if dev.type == "cuda" and dev.index is None:   # (the current one, as DeviceHandle reads it)
        dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if link.device != dev:
        raise ValueError(f"link lives on {link.device}, the env on {env.device}")
