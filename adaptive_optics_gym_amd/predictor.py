"""A predictive linear controller learnt on the device: the data-driven baseline learnt policies are read against.

``rollout(policy="ideal")`` applies a perfect measurement one frame late; the integrators (``"shack"``, ``"pyramid"``) are slower still.
``PredictiveController`` closes that lag with a per-env linear predictor of order ``p`` whose weights a recursive-least-squares (RLS) update
learns while the loop runs (``aog_predictor_update``, ``csrc/k_predictor.h``): from the last ``p`` pseudo-open-loop measurements — the
actuator vectors that would have flattened the wavefront at the steps they were taken — it predicts the one the NEXT screen will ask for,
and that prediction is the action.  It depends on no sensor: any such measurement feeds it (``update``); ``action`` takes one of the two the
device already has, ``wavefront_truth()["ideal_actuators"]`` (noise-free) or the pyramid sensor's ``a - R (s - s_ref)``
(``aog_pyramid_update`` with gain 1).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib
from .device_handle import DeviceHandle, check_measurement, ptr


class DevicePredictor(DeviceHandle):
    """The library handle (``aog_predictor``) alone: ``batch`` independent RLS predictors of ``act_dim`` outputs and ``order`` past
    measurements, float64 on ``device``.  ``update(y, mask=None)`` -> (prediction, innovation), both [batch, act_dim] float64.
    The state blob of ``get_state`` / ``set_state`` holds per env W [n, A], P [n, n], history [n] float64, count and skipped int64."""

    prefix, noun = "aog_predictor", "predictor"

    def __init__(self, batch, act_dim, order=2, forgetting=0.999, p0=1e3, scale=1.0, env_id_base=0, device=None):
        import torch

        self.batch, self.act_dim, self.order = int(batch), int(act_dim), int(order)
        self._bind(torch, device, self.batch)
        self.config = _lib.AogPredictorConfig(self.batch, self.act_dim, self.order, int(env_id_base), 0, 0, float(forgetting), float(p0), float(scale))
        self._create()

    def _config(self):
        return self.config

    def _rows(self, t, who, name):
        return self._tensor(t, (self.batch, self.act_dim), self._torch.float64,
                            f"{who}: {name} must be a contiguous float64 [{self.batch}, {self.act_dim}] tensor on {self.device}")

    def update(self, y, mask=None, out=None):
        """One RLS update and prediction per selected env.  ``out`` = (pred, innov) tensors to write into (rows of unselected envs are not
        written: fresh tensors hold zeros there)."""
        torch = self._torch
        y = self._rows(y, "update", "y")
        m = self._mask(mask, "update")
        if out is None:
            alloc = torch.empty if m is None else torch.zeros
            pred, innov = alloc_like(alloc, y), alloc_like(alloc, y)
        else:
            pred, innov = self._rows(out[0], "update", "out[0]"), self._rows(out[1], "update", "out[1]")
        self._call("update", ptr(y), ptr(m), ptr(pred), ptr(innov), self._stream())
        return pred, innov

    def reset(self, mask=None):
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    def unpack(self, blob=None):
        """A blob as a dict of tensors: W [B, n, A], P [B, n, n], history [B, n] float64, count [B], skipped [B] int64 (copies)."""
        torch = self._torch
        blob = self.get_state() if blob is None else blob
        n, A, B = self.act_dim * self.order, self.act_dim, self.batch
        words = blob.view(torch.float64).reshape(B, n * A + n * n + n + 2)
        ints = blob.view(torch.int64).reshape(B, -1)
        return {"W": words[:, :n * A].reshape(B, n, A).clone(), "P": words[:, n * A:n * A + n * n].reshape(B, n, n).clone(),
                "history": words[:, n * A + n * n:n * A + n * n + n].clone(), "count": ints[:, -2].clone(), "skipped": ints[:, -1].clone()}


def alloc_like(alloc, t):
    return alloc(t.shape, dtype=t.dtype, device=t.device)


def pseudo_open_loop(env, measurement, who):
    """The pseudo-open-loop measurement of ``env`` at the state the last ``reset`` / ``step`` left, [B, A] float64 actuators:
    ``"truth"``: ``env.ideal_action()``; ``"pyramid"``: the pyramid sensor's integrator with gain 1, ``a - R (s - s_ref)``."""
    if getattr(env, "_next_actions_keepalive", None) is not None:
        raise ValueError(f"{who}: a pipelined step has an action pending (the mirror already belongs to the next step)")
    try:
        if measurement == "truth":
            return env.ideal_action()
        torch = env._torch
        env._instrument_mask("pyramid", None, who)
        if not env._pyramid_calibrated:
            env.pyramid_calibrate()
        y = torch.empty((env.num_envs, env.num_modes), dtype=torch.float64, device=env.device)
        _lib.check(env.lib.aog_pyramid_update(env._handle, 1.0, C.c_void_p(y.data_ptr()), None, env._stream()))
        env.pyramid_frame_count += 1
        return y
    except _lib.AogError as err:
        if "NEXT action" in str(err) or "advanced to the next step" in str(err):
            raise ValueError(f"{who}: {err}") from None
        raise


class PredictiveController:
    """The predictive controller of an env (``BatchedAOEnv`` or ``LayeredAOEnv``).

    ``action()`` takes the pseudo-open-loop measurement from the env at the state the last ``reset`` / ``step`` left —
    ``measurement="truth"``: ``env.ideal_action()``; ``"pyramid"``: the pyramid sensor's integrator with gain 1, ``a - R (s - s_ref)`` —
    runs one RLS update and returns the prediction, [B, A] float64 actuators in the form ``SH_step()[0]`` and ``ideal_action()`` return
    (the action of an env built with ``SH_operation=True``).  ``update(y)`` does the same for a caller's own measurement.  The first
    ``order`` actions are the measurements themselves (``'ideal'``'s actions); after that every call first corrects the weights by what
    the last regressor mispredicted, then predicts.  ``innovation`` is the last call's prediction error (metres), ``measurement_value`` the
    measurement it took.  ``scale`` (default ``wavelength_wfs / 2 pi``, a radian of phase) only conditions the arithmetic: measurements are
    divided by it before they enter the regressor, so ``p0`` and ``forgetting`` mean the same at every wavelength.  The predictor is per env and keeps learning
    across episodes (the atmosphere is not reset either): ``reset(mask)`` is the caller's.  ``state_dict`` / ``load_state_dict`` resume bit-identically."""

    def __init__(self, env, order=2, forgetting=0.999, p0=1e3, scale=None, measurement="truth"):
        check_measurement(env, measurement)
        order = int(order)
        A = int(env.num_modes)
        if order < 1:
            raise ValueError(f"order must be >= 1 (got {order})")
        if scale is None:
            scale = float(env.wavelength_wfs) / (2.0 * math.pi)
        scale, forgetting, p0 = float(scale), float(forgetting), float(p0)
        if not (0.0 < forgetting <= 1.0):
            raise ValueError(f"forgetting must lie in (0, 1] (got {forgetting})")
        if not (math.isfinite(p0) and p0 > 0.0 and math.isfinite(scale) and scale > 0.0):
            raise ValueError(f"p0 and scale must be finite and > 0 (got {p0}, {scale})")
        self.env = env
        self.measurement = measurement
        self.order, self.forgetting, self.p0, self.scale = order, forgetting, p0, scale
        self.predictor = DevicePredictor(env.num_envs, A, order, forgetting, p0, scale, int(getattr(env, "global_env_offset", 0)), env.device)
        self.innovation = None
        self.measurement_value = None

    def _measure(self):
        return pseudo_open_loop(self.env, self.measurement, "PredictiveController.action")

    def action(self):
        return self.update(self._measure())

    def update(self, y, mask=None):
        pred, innov = self.predictor.update(y, mask)
        self.measurement_value, self.innovation = y, innov
        return pred

    def reset(self, mask=None):
        self.predictor.reset(mask)

    def state_dict(self):
        return {"blob": self.predictor.get_state(), "order": self.order, "act_dim": self.predictor.act_dim, "batch": self.predictor.batch,
                "forgetting": self.forgetting, "p0": self.p0, "scale": self.scale}

    def load_state_dict(self, state):
        for k in ("order", "forgetting", "p0", "scale"):
            if state[k] != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]}, this controller has {getattr(self, k)}")
        if state["act_dim"] != self.predictor.act_dim or state["batch"] != self.predictor.batch:
            raise ValueError("load_state_dict: the state belongs to another batch or act_dim")
        self.predictor.set_state(state["blob"])

    def close(self):
        self.predictor.close()
