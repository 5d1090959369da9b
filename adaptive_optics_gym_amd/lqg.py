"""An LQG controller: per-mode Kalman prediction of turbulence and vibration lines, on the device.

The integrator (``ModalIntegrator``) cannot notch a vibration line and loses gain with every frame of loop delay; the predictive controller
(``PredictiveController``) has to relearn every line from data.  The LQG controller models what it fights: per env and mode the
pseudo-open-loop measurement is ``y_t = sum_s x^(s)_t + w_t``, each sub-model an AR(2) process — sub-model 0 the turbulence, the others
the declared vibration lines, the form ``disturbance.ar2_parameters`` returns — and a steady-state Kalman filter on that state predicts
the measurement ``delay`` frames ahead; the prediction is the command.  The gains come from a fixed number of Riccati iterations on the
device (``aog_lqg_solve``), a frame is one launch (``aog_lqg_update``); ``include/aogym_lqg.h`` writes out the arithmetic,
``csrc/k_lqg.h`` runs it.

Not modelled: a mirror that answers with a first-order ``response`` < 1 (``servo.MirrorServo``), and a fractional servo latency — round
it up, as for ``ModalIntegrator``: ``delay = 1 + ceil(latency)``.
"""
from __future__ import annotations

import math

from . import _lib
from .device_handle import DeviceHandle, check_measurement, ptr
from .telemetry import MAX_DELAY

MAX_MODES, MAX_MODELS, MAX_ITERATIONS = _lib.LQG_MAX_ACT, _lib.LQG_MAX_MODELS, _lib.LQG_MAX_ITERATIONS
MIN_SAMPLES = 64          # identify_ar2: fewer samples in a ring give no fit
CONVERGED = 1e-9          # LQGController.solve: the largest relative change of trace P it accepts
VIBRATION_KEYS = {"frequency", "damping", "ratio"}


def check_delay(delay):
    d = int(delay)
    if d != delay or not 1 <= d <= MAX_DELAY:
        raise ValueError(f"delay must be 1, 2, 3 or 4 (got {delay!r})")
    return d


class DeviceLQG(DeviceHandle):
    """The library handle (``aog_lqg``) alone: ``batch`` x ``act_dim`` independent filters of ``n_models`` AR(2) sub-models, float64 on
    ``device``.  ``set_model(a, q, r)`` stores a model and drops the gains, ``solve(delay, iterations)`` -> convergence [batch, act_dim],
    ``update(y)`` -> the command [batch, act_dim] (``_lib.AogError`` before ``solve``), ``reset()`` zeroes the filter state and the command.
    The state blob of ``get_state`` / ``set_state`` is everything per env (``unpack``): a resumed handle needs no ``solve``."""

    prefix, noun = "aog_lqg", "LQG filter"

    def __init__(self, batch, act_dim, n_models, device=None):
        import torch

        self.batch, self.act_dim, self.n_models = int(batch), int(act_dim), int(n_models)
        if self.batch < 1:
            raise ValueError(f"DeviceLQG: num_envs must be >= 1, got {batch!r}")
        if not 1 <= self.act_dim <= MAX_MODES:
            raise ValueError(f"DeviceLQG: act_dim must lie in 1 .. {MAX_MODES}, got {act_dim!r}")
        if not 1 <= self.n_models <= MAX_MODELS:
            raise ValueError(f"DeviceLQG: n_models must lie in 1 .. {MAX_MODELS}, got {n_models!r}")
        self._bind(torch, device, self.batch)
        self._create()

    def _config(self):
        return _lib.AogLqgConfig(_lib.ABI_VERSION, self.batch, self.act_dim, self.n_models, 0)

    def _rows(self, t, who, name, *middle):
        shape = (self.batch,) + middle + (self.act_dim,)
        return self._tensor(t, shape, self._torch.float64, f"{who}: {name} must be a contiguous float64 {list(shape)} tensor on {self.device}")

    def set_model(self, a, q, r, mask=None):
        """a [batch, S, 2, A] (a1, a2), q [batch, S, A], r [batch, A]: the selected envs' model; their gains, filter state and command
        become zero.  Nothing is validated here: ``solve``'s convergence figure is NaN or large for a model that is not finite, is
        unstable or has r <= 0."""
        S = self.n_models
        a, q, r = self._rows(a, "set_model", "a", S, 2), self._rows(q, "set_model", "q", S), self._rows(r, "set_model", "r")
        self._call("set_model", ptr(a), ptr(q), ptr(r), ptr(self._mask(mask, "set_model")), self._stream())

    def solve(self, delay=1, iterations=256, mask=None, out=None):
        """``iterations`` Riccati steps, then K and c_d = C A^delay of the selected envs; returns |tr P_last - tr P_prev| / tr P_last
        [batch, act_dim] (rows of unselected envs are not written: a fresh tensor holds zeros there)."""
        torch = self._torch
        d, it = check_delay(delay), int(iterations)
        if it != iterations or not 1 <= it <= MAX_ITERATIONS:
            raise ValueError(f"solve: iterations must lie in 1 .. {MAX_ITERATIONS} (got {iterations!r})")
        m = self._mask(mask, "solve")
        out = torch.zeros((self.batch, self.act_dim), dtype=torch.float64, device=self.device) if out is None else self._rows(out, "solve", "out")
        self._call("solve", d, it, ptr(out), ptr(m), self._stream())
        return out

    def update(self, y, mask=None, out=None):
        """One frame of the selected envs; returns the command [batch, act_dim] of every env as it stands after the call.  A row of y with
        a non-finite value leaves its env as it was."""
        torch = self._torch
        y = self._rows(y, "update", "y")
        m = self._mask(mask, "update")
        out = torch.empty((self.batch, self.act_dim), dtype=torch.float64, device=self.device) if out is None else self._rows(out, "update", "out")
        self._call("update", ptr(y), ptr(out), ptr(m), self._stream())
        return out

    def reset(self, mask=None):
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    def unpack(self, blob=None):
        """A blob as a dict of float64 tensors (copies): a [B, S, 2, A], q [B, S, A], r [B, A], K [B, n, A], c [B, n, A],
        convergence [B, A], solved [B, A] (0 or 1), xhat [B, n, A], command [B, A]."""
        torch = self._torch
        blob = self.get_state() if blob is None else blob
        B, A, S = self.batch, self.act_dim, self.n_models
        n = 2 * S
        rows = blob.view(torch.float64).reshape(B, 9 * S + 4, A)
        cut = {"a": 2 * S, "q": S, "r": 1, "K": n, "c": n, "convergence": 1, "solved": 1, "xhat": n, "command": 1}
        out, at = {}, 0
        for name, count in cut.items():
            part = rows[:, at:at + count].clone()
            out[name] = part[:, 0] if name in ("r", "convergence", "solved", "command") else part
            at += count
        out["a"] = out["a"].reshape(B, S, 2, A)
        return out


# ---- identification: plain torch, device-agnostic ------------------------------------------------------------------------------------------
def ring_autocovariance(hist, count):
    """The mean-removed autocovariances at lags 0, 1, 2 of the samples a telemetry ring holds, in chronological order.

    hist [B, T, A] (sample number c sits in row c mod T), count [B] (samples pushed so far).  Returns (acov [B, 3, A], n [B]): n =
    min(count, T) samples, ``acov[:, k] = (1 / n) sum_{t >= k} (x_t - mean)(x_{t-k} - mean)`` over the chronological samples — no product
    pairs the newest sample with the oldest across the ring's write point.  n = 0 gives NaN."""
    import torch

    B, T, A = hist.shape
    count = torch.as_tensor(count, device=hist.device).to(torch.int64).clamp(min=0)
    n = count.clamp(max=T)
    start = torch.where(count > T, count % T, torch.zeros_like(count))
    t = torch.arange(T, device=hist.device)
    rows = (start[:, None] + t[None, :]) % T                                   # [B, T]: where chronological sample t sits
    x = torch.gather(hist, 1, rows[:, :, None].expand(B, T, A))
    live = (t[None, :] < n[:, None]).to(hist.dtype)[:, :, None]                 # [B, T, 1]
    nf = n.to(hist.dtype)[:, None]
    mean = (x * live).sum(dim=1) / nf
    d = (x - mean[:, None, :]) * live
    acov = torch.stack([(d * d).sum(dim=1), (d[:, 1:] * d[:, :-1]).sum(dim=1), (d[:, 2:] * d[:, :-2]).sum(dim=1)], dim=1) / nf[:, None, :]
    return acov, n


def ar2_autocovariance(a1, a2, q):
    """[B, 3, A]: the autocovariances at lags 0, 1, 2 of the stationary AR(2) processes (a1, a2, q), [B, A] tensors each."""
    import torch

    var = q * (1.0 - a2) / ((1.0 + a2) * ((1.0 - a2) ** 2 - a1 ** 2))
    rho1 = a1 / (1.0 - a2)
    return torch.stack([var, var * rho1, var * (a1 * rho1 + a2)], dim=1)


def identify_ar2(hist, count, lines_acov=None, noise_var=0.0):
    """Fit the turbulence sub-model to a telemetry ring by Yule-Walker.

    hist [B, T, A], count [B] as ``ModalTelemetry.unpack()`` gives them; lines_acov [B, 3, A] or None: the autocovariances at lags 0, 1, 2
    of everything else the model declares (the vibration lines), subtracted before the fit; noise_var (a number or [B, A]): the
    measurement noise, subtracted at lag 0.  Returns (a1, a2, q, valid), [B, A] each: ``[c0 c1; c1 c0] [a1; a2] = [c1; c2]``,
    ``q = c0 - a1 c1 - a2 c2``; ``valid`` is False where the ring holds fewer than 64 samples, where a root of z^2 - a1 z - a2 lies on or
    outside the unit circle, where q <= 0 or where a value is not finite — such entries keep the model they have."""
    import torch

    acov, n = ring_autocovariance(hist, count)
    if lines_acov is not None:
        acov = acov - lines_acov
    c0, c1, c2 = acov[:, 0] - noise_var, acov[:, 1], acov[:, 2]
    det = c0 * c0 - c1 * c1
    a1 = c1 * (c0 - c2) / det
    a2 = (c0 * c2 - c1 * c1) / det
    q = c0 - a1 * c1 - a2 * c2
    stable = (a2.abs() < 1.0) & (a1 + a2 < 1.0) & (a2 - a1 < 1.0)
    finite = torch.isfinite(a1) & torch.isfinite(a2) & torch.isfinite(q)
    valid = (n >= MIN_SAMPLES)[:, None] & stable & finite & (q > 0.0)
    return a1, a2, q, valid


# ---- the controller ------------------------------------------------------------------------------------------------------------------------
def _per_mode(value, A, what):
    """A scalar or [A] values as a float64 numpy vector [A]."""
    import numpy as np

    v = np.asarray(value, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(A, float(v))
    if v.shape != (A,) or not np.all(np.isfinite(v)) or np.any(v < 0.0):
        raise ValueError(f"{what} must be a finite number >= 0 or one per mode ([{A}]) (got {value!r})")
    return v


def default_model(B, A, vibrations=(), turbulence_pole=0.99, noise_ratio=1e-2):
    """The model before any identification, as numpy arrays a [B, S, 2, A], q [B, S, A], r [B, A] and the lines' ratios [L, A]: the
    turbulence an AR(2) with a double pole at ``turbulence_pole`` and unit variance, r = ``noise_ratio``, every line
    ``dict(frequency=cycles per frame, damping=, ratio=variance relative to the turbulence, a number or one per mode)`` through
    ``disturbance.ar2_parameters(delta_t=1)``.  Only the ratios matter to the gains."""
    import numpy as np

    from .disturbance import ar2_parameters

    vibrations = list(vibrations)
    if len(vibrations) > MAX_MODELS - 1:
        raise ValueError(f"vibrations: at most {MAX_MODELS - 1} lines (got {len(vibrations)})")
    pole, noise_ratio = float(turbulence_pole), float(noise_ratio)
    if not 0.0 < pole < 1.0:
        raise ValueError(f"turbulence_pole must lie in (0, 1) (got {turbulence_pole!r})")
    if not (math.isfinite(noise_ratio) and noise_ratio > 0.0):
        raise ValueError(f"noise_ratio must be finite and > 0 (got {noise_ratio!r})")
    S = 1 + len(vibrations)
    a, q, ratios = np.zeros((B, S, 2, A)), np.zeros((B, S, A)), np.zeros((len(vibrations), A))
    a1, a2 = 2.0 * pole, -pole * pole
    a[:, 0, 0], a[:, 0, 1] = a1, a2
    q[:, 0] = (1.0 + a2) * ((1.0 - a2) ** 2 - a1 ** 2) / (1.0 - a2)      # unit variance
    for k, v in enumerate(vibrations):
        if not isinstance(v, dict) or set(v) != VIBRATION_KEYS:
            raise ValueError("vibrations: every entry is a dict with exactly the keys 'frequency', 'damping' and 'ratio'")
        ratios[k] = _per_mode(v["ratio"], A, f"vibrations[{k}].ratio")
        p = ar2_parameters(v["frequency"], v["damping"], 1.0, 1.0)     # (frequency in cycles per frame: delta_t = 1)
        a[:, k + 1, 0], a[:, k + 1, 1] = p["a1"], p["a2"]
        q[:, k + 1] = p["b"] ** 2 * ratios[k]
    return a, q, np.full((B, A), noise_ratio), ratios


class LQGController:
    """The LQG controller of an env (``BatchedAOEnv`` or ``LayeredAOEnv``).

    ``action()`` takes the pseudo-open-loop measurement y exactly as ``ModalIntegrator`` does (``measurement="truth"``:
    ``env.ideal_action()``; ``"pyramid"``: the pyramid integrator at gain 1) and returns ``update(y)``: y goes into ``telemetry`` (a
    ``ModalTelemetry``, made here unless one is passed) and through one Kalman update; the command is the filter's prediction of the
    measurement ``delay`` frames ahead, [B, A] float64 actuators in the form ``ideal_action()`` returns.  A row of y with a non-finite
    value leaves its env's filter and command as they were.  ``delay`` is the lag, in frames, between a measurement and the command it
    yields reaching the mirror: 1 in ``rollout``'s loop, ``1 + latency`` for an env built with ``servo=dict(latency=...)`` (round a
    fractional latency up; a mirror ``response`` < 1 is not modelled).

    The model (``default_model``): the turbulence an AR(2) with a double pole at ``turbulence_pole``, measurement noise ``noise_ratio``
    of its variance, and per entry of ``vibrations`` a line ``dict(frequency=cycles per frame, damping=, ratio=variance relative to the
    turbulence)``, at most three.  ``set_model(a, q, r)`` takes the caller's own [B, S, 2, A], [B, S, A] and [B, A] tensors instead.
    The constructor solves the default model; after ``set_model`` or ``identify`` call ``solve()``: it returns the convergence figure
    [B, A] and raises ``ValueError`` naming the worst (env, mode) if a selected entry is NaN or above 1e-9.
    ``identify(noise_var=0.0, mask=None)`` refits the turbulence sub-model from the controller's own telemetry ring (``identify_ar2``)
    and returns ``valid`` [B, A]; entries that are not valid keep their model.  ``reset(mask)`` zeroes the filter state and the command
    and empties the telemetry; the model and gains stay.  ``state_dict`` / ``load_state_dict`` resume bit-identically without solving
    again; everything runs on the caller's current stream."""

    def __init__(self, env, measurement="truth", delay=1, vibrations=(), turbulence_pole=0.99, noise_ratio=1e-2, iterations=256, telemetry=None):
        check_measurement(env, measurement)
        self.delay = check_delay(delay)
        self.iterations = int(iterations)
        if self.iterations != iterations or not 1 <= self.iterations <= MAX_ITERATIONS:
            raise ValueError(f"iterations must lie in 1 .. {MAX_ITERATIONS} (got {iterations!r})")
        B, A = int(env.num_envs), int(env.num_modes)
        a, q, r, self.ratios = default_model(B, A, vibrations, turbulence_pole, noise_ratio)
        self.noise_ratio = float(noise_ratio)
        from .telemetry import ModalTelemetry

        if telemetry is None:
            telemetry = ModalTelemetry(B, A, device=env.device, global_env_offset=int(getattr(env, "global_env_offset", 0)))
        elif (telemetry.num_envs, telemetry.act_dim) != (B, A):
            raise ValueError(f"telemetry holds [{telemetry.num_envs}, {telemetry.act_dim}] measurements, the env gives [{B}, {A}]")
        import torch

        self.env, self.measurement, self.telemetry = env, measurement, telemetry
        self.n_models = a.shape[1]
        self.filter = DeviceLQG(B, A, self.n_models, telemetry.device)
        dev = self.filter.device
        self.a, self.q, self.r = (torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous() for v in (a, q, r))
        self.measurement_value = None
        self.filter.set_model(self.a, self.q, self.r)
        self.convergence = self.solve()

    # -- the model --
    def set_model(self, a, q, r, mask=None):
        """The caller's own model for the selected envs (``DeviceLQG.set_model``'s shapes); ``solve()`` must follow."""
        self.filter.set_model(a, q, r, mask)
        torch = self.filter._torch
        if mask is None:
            self.a, self.q, self.r = a.clone(), q.clone(), r.clone()
        else:
            m = torch.as_tensor(mask, device=a.device).to(torch.bool)
            self.a[m], self.q[m], self.r[m] = a[m], q[m], r[m]

    def solve(self, mask=None):
        torch = self.filter._torch
        conv = self.filter.solve(self.delay, self.iterations, mask)
        looked = conv if mask is None else conv[torch.as_tensor(mask, device=conv.device).to(torch.bool)]
        bad = torch.isnan(looked) | (looked > CONVERGED)
        if bool(bad.any()):
            worst = torch.where(torch.isnan(conv), torch.full_like(conv, float("inf")), conv)
            if mask is not None:
                worst = torch.where(torch.as_tensor(mask, device=conv.device).to(torch.bool)[:, None], worst, torch.full_like(conv, -1.0))
            at = int(worst.argmax())
            b, j = divmod(at, conv.shape[1])
            raise ValueError(f"LQGController.solve: the Riccati recursion of env {b}, mode {j} has not converged after {self.iterations} iterations "
                             f"(relative change of trace P {float(conv[b, j])!r}, limit {CONVERGED:g}): the model is not finite, is unstable, has "
                             "r <= 0, or needs more iterations")
        self.convergence = conv
        return conv

    def identify(self, noise_var=0.0, mask=None):
        """Refit the turbulence sub-model of the selected envs from the telemetry ring: the declared lines' share of the ring's variance
        (their ``ratio``) and ``noise_var`` are subtracted, Yule-Walker gives a1, a2 and q, the lines' q are scaled to their ratio of the
        fitted turbulence variance, and r becomes ``noise_var`` (``noise_ratio`` of that variance when ``noise_var`` is 0).  Returns
        ``valid`` [B, A]; envs with a valid entry get the new model and lose their gains and filter state: call ``solve()``."""
        torch = self.filter._torch
        state = self.telemetry.unpack()
        hist, count = state["hist"], state["count"]
        acov, _ = ring_autocovariance(hist, count)
        ratios = torch.as_tensor(self.ratios, dtype=torch.float64, device=hist.device)                # [L, A]
        turb_var = (acov[:, 0] - noise_var) / (1.0 + ratios.sum(dim=0))[None, :]                       # [B, A]
        lines = None
        line_q = []
        for k in range(self.n_models - 1):
            a1, a2 = self.a[:, k + 1, 0], self.a[:, k + 1, 1]
            unit = ar2_autocovariance(a1, a2, torch.ones_like(a1))                                     # per unit of q
            qk = turb_var * ratios[k][None, :] / unit[:, 0]
            line_q.append(qk)
            part = unit * qk[:, None, :]
            lines = part if lines is None else lines + part
        a1, a2, q, valid = identify_ar2(hist, count, lines, noise_var)
        if mask is not None:
            valid = valid & torch.as_tensor(mask, device=valid.device).to(torch.bool)[:, None]
        new_a, new_q, new_r = self.a.clone(), self.q.clone(), self.r.clone()
        new_a[:, 0, 0] = torch.where(valid, a1, self.a[:, 0, 0])
        new_a[:, 0, 1] = torch.where(valid, a2, self.a[:, 0, 1])
        new_q[:, 0] = torch.where(valid, q, self.q[:, 0])
        for k, qk in enumerate(line_q):
            new_q[:, k + 1] = torch.where(valid, qk, self.q[:, k + 1])
        fitted_r = torch.full_like(turb_var, float(noise_var)) if float(noise_var) > 0.0 else self.noise_ratio * turb_var
        new_r = torch.where(valid, fitted_r, self.r)
        envs = valid.any(dim=1)
        if bool(envs.any()):
            self.set_model(new_a.contiguous(), new_q.contiguous(), new_r.contiguous(), envs)
        return valid

    # -- the loop --
    def action(self):
        from .predictor import pseudo_open_loop

        return self.update(pseudo_open_loop(self.env, self.measurement, "LQGController.action"))

    def update(self, y, mask=None):
        self.telemetry.push(y, mask)
        self.measurement_value = y
        return self.filter.update(y, mask)

    @property
    def command(self):
        """[B, A] float64: the command this controller last returned."""
        return self.filter.unpack()["command"]

    def reset(self, mask=None):
        """The selected envs' filter state and command back to zero and their telemetry emptied (the model and the gains stay)."""
        self.telemetry.reset(mask)
        self.filter.reset(mask)

    def state_dict(self):
        return {"telemetry": self.telemetry.state_dict(), "blob": self.filter.get_state(), "a": self.a.clone(), "q": self.q.clone(), "r": self.r.clone(),
                "delay": self.delay, "n_models": self.n_models, "batch": self.filter.batch, "act_dim": self.filter.act_dim}

    def load_state_dict(self, state):
        for k, have in (("delay", self.delay), ("n_models", self.n_models), ("batch", self.filter.batch), ("act_dim", self.filter.act_dim)):
            if state[k] != have:
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]}, this controller has {have}")
        self.telemetry.load_state_dict(state["telemetry"])
        self.filter.set_state(state["blob"])
        dev = self.a.device
        self.a, self.q, self.r = (state[k].to(dev).clone() for k in ("a", "q", "r"))

    def close(self):
        self.telemetry.close()
        self.filter.close()
