"""``LayeredAOEnv`` — a multi-layer frozen-flow atmosphere: several wind layers per env.

A single frozen-flow screen is a pure translation; a site has a slow ground layer and fast high layers moving in other directions, and
their sum is what makes a one-frame control lag cost Strehl.  On axis and conjugated to the pupil, L layers are exactly the sum of L
independent screens, so every layer here is an ordinary dynamic ``BatchedAOEnv`` that only evolves (``evolve_atmosphere``), one kernel
sums the layers' float64 master screens into the screen tiles of a quasi-static FRONT handle (``install_layer_sum``), and the front
steps with the static fused kernel it already has.  Everything that reads the front's screens — reset, step, the separable observation
route, Shack-Hartmann, ``wavefront_truth``, the science camera, ``output_gradient``, ``step_with_policy``, ``step_with_spgd``, pipelined steps — works on it
unchanged.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .batched_env import BatchedAOEnv, _mask_array
from .params import resolve_per_env, resolve_turbulence

MAX_LAYERS = 8   # aog_install_layer_sum's limit


def layer_seed(seed, layer):
    """The seed of layer ``layer``'s own env — the one place it is derived.  Layer 0 takes the env's ``seed`` unchanged (a one-layer env
    draws what a plain dynamic env with that seed draws); layer l > 0 takes the first 31-bit word of
    ``numpy.random.SeedSequence([base, l])``, base = ``seed`` (1234 when None, as ``BatchedAOEnv``): a hash, so that it collides neither
    with another layer's nor with the ``seed + global env id`` streams of the envs."""
    if layer == 0:
        return seed
    base = 1234 if seed is None else int(seed)
    return int(np.random.SeedSequence([base & 0xFFFFFFFFFFFFFFFF, int(layer)]).generate_state(1)[0] & 0x7FFFFFFF)


def resolve_layers(atm_layers, atm_fried, num_envs, total_envs=None, global_env_offset=0):
    """``atm_layers`` checked and split: a list of dict(fraction, fried, speed) — what layer l's env is built with.  ``atm_layers``:
    1 .. 8 of ``{"fraction": f_l, "speed": v_l}``; the fractions of the turbulence strength are positive and sum to 1 within 1e-12, each
    speed is a scalar or per-env values under ``atm_vel``'s rules.  Layer l runs at r0_l = r0 f_l^(-3/5) (per env when ``atm_fried`` is),
    so that the layers' Cn^2 add up to the Cn^2 of the requested r0 (Cn^2 is proportional to r0^(-5/3)).  ``ValueError`` for anything
    else, before anything is created."""
    total_envs = global_env_offset + num_envs if total_envs is None else int(total_envs)
    if atm_layers is None or isinstance(atm_layers, dict) or not 1 <= len(atm_layers) <= MAX_LAYERS:
        raise ValueError(f"atm_layers: expected a list of 1 .. {MAX_LAYERS} dicts {{'fraction': f, 'speed': v}}")
    fractions = []
    for lay in atm_layers:
        if not isinstance(lay, dict) or set(lay) != {"fraction", "speed"}:
            raise ValueError("atm_layers: every layer is a dict with exactly the keys 'fraction' and 'speed'")
        f = float(lay["fraction"])
        if not np.isfinite(f) or f <= 0:
            raise ValueError(f"atm_layers: fractions must be positive and finite, got {lay['fraction']!r}")
        fractions.append(f)
    if abs(float(np.sum(fractions)) - 1.0) > 1e-12:
        raise ValueError(f"atm_layers: the fractions must sum to 1 within 1e-12, got {float(np.sum(fractions))!r}")
    resolve_turbulence("dynamic", atm_fried, 1, num_envs, total_envs, global_env_offset, False)   # (the total r0's own checks)
    fried = np.asarray(atm_fried, dtype=np.float64)
    out = []
    for f, lay in zip(fractions, atm_layers):
        fried_l = fried * f ** (-3.0 / 5.0)
        fried_l = float(fried_l) if fried_l.ndim == 0 else fried_l
        resolve_turbulence("dynamic", fried_l, lay["speed"], num_envs, total_envs, global_env_offset, False)
        out.append(dict(fraction=f, fried=fried_l, speed=lay["speed"]))
    return out


class LayeredAOEnv(BatchedAOEnv):
    """``BatchedAOEnv`` over a layered dynamic atmosphere.  Keywords as ``BatchedAOEnv`` (``atm_type`` is 'dynamic'; ``atm_vel`` and
    ``screens`` do not apply) plus

    atm_layers   [{"fraction": f_l, "speed": v_l}, ...], 1 .. 8 layers (``resolve_layers``); ``atm_fried`` is the r0 of their sum.
    disturbance  None, or dict(shapes=, vibrations=, static=) for a ``disturbance.ModalDisturbance``: vibration lines and static
                 aberrations on K <= 8 pupil shapes, advanced once per step and added inside the layer sum (so everything that reads the
                 front sees them).  ``env.disturbance`` is the object; ``get_state`` / ``set_state`` carry its state; ``set_turbulence`` and
                 ``reset`` leave it alone.  Without it the env runs exactly the launches it ran before.

    Layer l is a private dynamic env with a seed of its own (``layer_seed``) and therefore wind directions and stencil draws of its own,
    as the reference draws them per layer; it shares this env's tables, ``extrusion``, ``screen_source`` and global env ids.  ``reset`` is
    the front's (the atmosphere is observed as it stands, like the reference's dynamic reset); ``step`` / ``step_with_policy`` first evolve
    every layer and install their sum, then step the front.  ``get_screens()`` is the float64 sum, ``layer_screens(l)`` one layer;
    ``velocity_vectors`` is [L, B, 2]; ``set_turbulence`` splits the new r0 by the same fractions; ``get_state`` / ``set_state`` carry the
    front's state and every layer's.  ``lookahead`` is not available (returns False) and ``set_screens`` raises.  ``obs_gradient`` goes to the
    front, an ordinary static handle: ``output_gradient`` differentiates the observation of the installed sum."""

    def __init__(self, num_envs=1, device=None, atm_layers=None, atm_fried=0.15, act_type="num_actuators", act_dim=64, obs_dim=2,
                 rew_type="strehl_ratio", rew_threshold=None, timesteps_per_episode=20, flat_mirror_start_per_episode=True, SH_operation=False, *,
                 atm_type="dynamic", seed=None, screen_source="device", rng=None, global_env_offset=0, total_envs=None, extrusion="auto",
                 verbose=True, disturbance=None, **kw):
        self._layers = []
        self._handle = None
        self.disturbance = None
        if atm_type != "dynamic":
            raise ValueError("LayeredAOEnv: atm_type is 'dynamic' (a layered atmosphere evolves every step)")
        for bad in ("atm_vel", "screens"):
            if bad in kw:
                raise ValueError(f"LayeredAOEnv: {bad} does not apply (every layer has its own speed and draws its own screens)")
        plan = resolve_layers(atm_layers, atm_fried, int(num_envs), total_envs, int(global_env_offset))
        # The front: a quasi-static handle whose screens are installed, never drawn (_generate_screens below is a no-op); it consumes no
        # host random draws, so layer 0 sees the streams a plain dynamic env with the same seed sees.
        super().__init__(num_envs, device, "quasi_static", 0, atm_fried, act_type, act_dim, obs_dim, rew_type, rew_threshold, timesteps_per_episode,
                         flat_mirror_start_per_episode, SH_operation, seed=seed, screen_source="device", rng=None,
                         global_env_offset=global_env_offset, total_envs=total_envs, extrusion=extrusion, verbose=verbose, **kw)
        self.atm_type = "dynamic"
        self.screen_source = screen_source
        self.layer_fractions = np.array([p["fraction"] for p in plan])
        layer_kw = {k: kw[k] for k in ("screen_oversampling", "precision", "kernel", "pixel_chunks", "screen_method") if k in kw}
        try:
            for i, p in enumerate(plan):
                # (timesteps_per_episode = 0: a layer is never reset, and the int8 extrusion only works ahead inside an episode)
                self._layers.append(BatchedAOEnv(self.num_envs, self.device, "dynamic", p["speed"], p["fried"], act_type, act_dim, obs_dim, rew_type,
                                                 None, 0, True, False, params=self.params, seed=layer_seed(seed, i), screen_source=screen_source,
                                                 rng=rng, global_env_offset=self.global_env_offset, total_envs=self.total_envs,
                                                 tables=self.tables, extrusion=extrusion, verbose=False, **layer_kw))
            self.velocity_vectors = np.stack([lay.velocity_vectors for lay in self._layers])   # [L, B, 2] m/s
            self.velocity = [lay.velocity for lay in self._layers]
            if disturbance is not None:
                self._attach_disturbance(disturbance)
            self._install()   # the first reset sees t = 0
        except Exception:
            self.close()
            raise

    num_layers = property(lambda self: len(self._layers))

    @property
    def wind_speeds(self):
        """[L, B] float64 wind speed of every layer and env."""
        return np.stack([lay.wind_speeds for lay in self._layers])

    def _generate_screens(self, mask=None):
        """The front draws no screens: its layers do (at construction and in ``set_turbulence``)."""

    def _push_turbulence(self):
        """Nor does its handle need the per-env Cn^2 (only screen synthesis and the extrusion read them)."""

    def _host_extrusion_noise(self):
        """The layers draw their own normals (``evolve_atmosphere``)."""

    def _attach_disturbance(self, disturbance):
        """``disturbance``: dict(shapes=, vibrations=, static=[, seed=]) for a ``ModalDisturbance`` of this env, or such an object made for
        this env's batch, global env ids and device.  Its basis goes to the front; from here on every installation is the disturbed form."""
        from .disturbance import ModalDisturbance

        if isinstance(disturbance, dict):
            if not set(disturbance) <= {"shapes", "vibrations", "static", "seed"} or "shapes" not in disturbance:
                raise ValueError("disturbance: a dict with 'shapes' and, optionally, 'vibrations', 'static' and 'seed'")
            disturbance = ModalDisturbance(self, **disturbance)
        elif not isinstance(disturbance, ModalDisturbance):
            raise ValueError("disturbance: a dict(shapes=, vibrations=, static=) or a ModalDisturbance")
        d = disturbance
        index = self.device.index if self.device.index is not None else self._torch.cuda.current_device()
        if d.device.index != index or d.num_envs != self.num_envs or d.global_env_offset != self.global_env_offset:
            raise ValueError(f"disturbance: made for {d.num_envs} envs from global id {d.global_env_offset} on {d.device}, this env has "
                             f"{self.num_envs} from {self.global_env_offset} on {self.device}")
        if d.basis.shape[1] != int(self.tables.n_ap):
            raise ValueError(f"disturbance: its shapes cover {d.basis.shape[1]} aperture pixels, this env's pupil has {int(self.tables.n_ap)}")
        d.upload_basis(self)
        self.disturbance = d
        self._coeff = d.coefficients()

    def _install(self):
        if self.disturbance is None:
            self.install_layer_sum(self._layers)
        else:
            self.install_layer_sum_disturbed(self._layers, self._coeff)

    def install_layer_sum_disturbed(self, layers, coeff):
        """``install_layer_sum`` with ``sum_k coeff[b][k] shape_k`` added inside the float64 sum (``aog_install_layer_sum_disturbed``; the
        shapes are those last uploaded with ``ModalDisturbance.upload_basis``).  ``coeff``: [B, K] float64 device tensor, metres of optical path."""
        torch = self._torch
        if not isinstance(coeff, torch.Tensor) or coeff.dtype != torch.float64 or coeff.dim() != 2 or coeff.shape[0] != self.num_envs or not coeff.is_contiguous():
            raise ValueError(f"install_layer_sum_disturbed: coeff must be a contiguous float64 [{self.num_envs}, K] device tensor")
        handles = (C.c_void_p * len(layers))(*[lay._handle.value for lay in layers])
        _lib.check(self.lib.aog_install_layer_sum_disturbed(self._handle, handles, len(layers), C.c_void_p(coeff.data_ptr()), int(coeff.shape[1]),
                                                            self._stream()))
        self.state_epoch += 1

    def _advance(self):
        for lay in self._layers:
            lay.evolve_atmosphere()
        if self.disturbance is not None:
            self._coeff = self.disturbance.advance()
        self._install()

    def step(self, actions, out=None, next_actions=BatchedAOEnv._PIPELINE_END):
        self._advance()
        return super().step(actions, out=out, next_actions=next_actions)

    def step_with_policy(self, policy, cov_var=0.5, out=None, policy_out=None, action=None, ou_noise=None, action_mode="sample"):
        self._advance()
        return super().step_with_policy(policy, cov_var, out=out, policy_out=policy_out, action=action, ou_noise=ou_noise, action_mode=action_mode)

    def step_with_spgd(self, ctrl, out=None, action=None, action_out=None):
        self._advance()
        return super().step_with_spgd(ctrl, out=out, action=action, action_out=action_out)

    def evolve_atmosphere(self):
        raise RuntimeError("LayeredAOEnv: the layers evolve inside step()")

    def lookahead(self, enable=True):
        return False

    def set_screens(self, screens, first=0):
        raise RuntimeError("LayeredAOEnv: the screens are the sum of the layers'; there is nothing to install")

    def set_extrusion_noise(self, noise):
        raise RuntimeError("LayeredAOEnv: hand each layer its normals (env.layers[l].set_extrusion_noise)")

    @property
    def layers(self):
        """The layers' envs (read their ``velocity_vectors`` / ``get_screens()``, or hand one its extrusion normals; do not step them)."""
        return tuple(self._layers)

    def layer_screens(self, layer, first=0, count=None):
        """Current float64 master screens of one layer: [count, N, N]."""
        return self._layers[layer].get_screens(first, count)

    def get_screens(self, first=0, count=None):
        """The float64 sum of the layers' screens in layer order (what ``install_layer_sum`` forms before it removes the aperture mean)."""
        total = self._layers[0].get_screens(first, count)
        for lay in self._layers[1:]:
            total = total + lay.get_screens(first, count)
        return total

    def set_turbulence(self, fried, mask=None):
        """New total r0 for the envs ``mask`` selects: every layer gets r0 f_l^(-3/5) and redraws those envs' screens now."""
        fried, _, _ = resolve_per_env("fried", fried, self.num_envs, self.total_envs, self.global_env_offset)
        if np.any(fried <= 0):
            raise ValueError("set_turbulence: Fried parameters must be > 0")
        sel = _mask_array(mask, self.num_envs, "set_turbulence")
        new = self._fried.copy()
        new[sel] = fried[sel]
        self._apply_fried(new)   # (raises before any layer changed when r0 is below what the extrusion tables were made for)
        for lay, f in zip(self._layers, self.layer_fractions):
            lay.set_turbulence(new * f ** (-3.0 / 5.0), mask)
        self._install()

    def get_state(self):
        state = super().get_state()
        state["layers"] = [lay.get_state() for lay in self._layers]
        if self.disturbance is not None:
            state["disturbance"] = self.disturbance.state_dict()
        return state

    def set_state(self, state):
        if len(state.get("layers", ())) != len(self._layers):
            raise ValueError("set_state: the state was saved with another number of layers")
        if ("disturbance" in state) != (self.disturbance is not None):
            raise ValueError("set_state: the state was saved " + ("with" if "disturbance" in state else "without") + " a disturbance, this env was built "
                             + ("without" if self.disturbance is None else "with") + " one")
        for lay, st in zip(self._layers, state["layers"]):
            lay.set_state(st)
        if self.disturbance is not None:
            self.disturbance.load_state_dict(state["disturbance"])
            self._coeff = self.disturbance.coefficients()
        super().set_state(state)
        self._install()   # (the front's blob holds the same tiles; installing again keeps one path)

    def close(self):
        for lay in self.__dict__.get("_layers", ()):
            lay.close()
        self._layers = []
        if self.__dict__.get("disturbance") is not None:
            self.disturbance.close()
            self.disturbance = None
        super().close()
