"""Batched data collection over ``BatchedAOEnv`` — the device-resident counterpart of the reference's
``ALGORITHM.rollout`` (``algorithm.py:216-296``) and of the policy query it makes per step (``network.py:62-69``).

What is mirrored, and what is not:

* episode structure: ``reset()``, then ``timesteps_per_episode`` steps, break on ``done`` (``algorithm.py:238-276``) — here
  all envs run in lock-step because ``done`` depends only on the step counter (``AO_env.py:147``);
* the action is ``mean + N(0, 0.5 I)`` (``cov_var = 0.5``, ``algorithm.py:107-108``) from a 3-hidden-layer ReLU MLP whose
  dropout (p = 0.5) stays ACTIVE while acting (``network.py:39,48-55``; the reference never calls ``eval()``);
* batch layout ``(T*E, ...)`` per env (``algorithm.py:219-226``) gains a leading env axis: ``[T*E, B, ...]``;
* the logged scalar is ``mean(sum(ep_rew)) / T`` (``algorithm.py:509-510``), here over all envs of all ranks via one
  all-gather of episode returns per episode (``sharding.EpisodeReturnGatherer``).

The learners (SAC/DDPG/PPO updates, replay buffer) are outside the env hot path and are not rebuilt; the tensors returned
here are what they consume: ``replay_transitions`` flattens them into the five arrays the reference's replay buffer stores and
samples (``replay_buffer.py:21-34``: state, action, reward, next_state, done), ``sharding.gather_transitions`` all-gathers them over
the ranks for a central buffer.
"""
from __future__ import annotations

import math
import weakref
from collections import namedtuple


def make_actor(state_dim: int, act_dim: int, hidden_dim: int, init_w: float = 3e-3, device=None):
    """An MLP with the reference Actor's shape and initialisation ranges (``network.py:17-39``)."""
    import torch
    from torch import nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            dims = [(state_dim, hidden_dim), (hidden_dim, hidden_dim), (hidden_dim, hidden_dim)]
            self.hidden = nn.ModuleList(nn.Linear(i, o) for i, o in dims)
            for layer, (i, _) in zip(self.hidden, dims):
                bound = 1.0 / math.sqrt(i)
                nn.init.uniform_(layer.weight, -bound, bound)
                nn.init.uniform_(layer.bias, -bound, bound)
            self.out = nn.Linear(hidden_dim, act_dim)
            nn.init.uniform_(self.out.weight, -init_w, init_w)
            nn.init.uniform_(self.out.bias, -init_w, init_w)
            self.dropout = nn.Dropout(0.5)

        def forward(self, obs):
            x = obs.to(torch.float32)
            for layer in self.hidden:
                x = self.dropout(torch.relu(layer(x)))
            return self.out(x)

    actor = Actor()
    actor.train()  # dropout stays on while acting, like the reference
    return actor.to(device) if device is not None else actor


def sample_action(mean, cov_var: float = 0.5, generator=None):
    """``MultivariateNormal(mean, cov_var * I).rsample()`` and its log-probability, batched."""
    import torch

    std = math.sqrt(cov_var)
    eps = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
    action = mean + std * eps
    k = mean.shape[-1]
    log_prob = -0.5 * (eps * eps).sum(-1) - 0.5 * k * math.log(2 * math.pi * cov_var)
    return action, log_prob


def actor_layers(actor):
    """The four ``nn.Linear`` of a policy module in forward order, or None.  Two structures are recognised by ATTRIBUTE NAME: the reference's own
    ``Actor`` (``network.py:17-39``: ``layer1a``, ``layer2a``, ``layer3a``, ``outputa``) — so ``rollout(env, reference_actor)`` takes the fused
    kernel like any other — and ``make_actor``'s (``hidden`` = three layers, ``out``)."""
    names = ("layer1a", "layer2a", "layer3a", "outputa")
    if all(hasattr(actor, n) for n in names):
        return [getattr(actor, n) for n in names]
    if hasattr(actor, "hidden") and hasattr(actor, "out") and len(list(actor.hidden)) == 3:
        return list(actor.hidden) + [actor.out]
    return None


class OrnsteinUhlenbeckNoise:
    """DDPG's exploration noise (``network.py:259-274``; added to the action at ``algorithm.py:258-259``) for a batch of envs on the device:
    ``state += theta (mu - state) + sigma N(0, I)``; ``sample`` returns the state itself.  One independent process per env
    (the reference has one env, hence one process); ``reset`` puts every state back to ``mu``.  Like the reference's it is NOT reset between
    episodes unless the caller does so."""

    def __init__(self, num_envs: int, action_dim: int, mu: float, theta: float, sigma: float, device=None, generator=None):
        import torch

        self.mu, self.theta, self.sigma = float(mu), float(theta), float(sigma)
        self.generator = generator
        self.state = torch.full((int(num_envs), int(action_dim)), self.mu, dtype=torch.float32, device=device)

    def reset(self):
        self.state.fill_(self.mu)

    def sample(self):
        import torch

        eps = torch.randn(self.state.shape, dtype=self.state.dtype, device=self.state.device, generator=self.generator)
        self.state += self.theta * (self.mu - self.state) + self.sigma * eps
        return self.state


class DeviceOUNoise:
    """DDPG's exploration noise (``network.py:259-274``, ``algorithm.py:258-259``) advanced INSIDE the HIP policy query (``aog_action_noise``):
    a float64 state ``[num_envs, action_dim]`` on the device, like the reference's ``np.ones(...) * mu``, that every query it is passed to
    (``DeviceActor(..., ou_noise=)``, ``BatchedAOEnv.reset_with_policy`` / ``step_with_policy(..., ou_noise=)``, ``rollout(..., ou_noise=)``)
    advances once: ``s = s + (theta (mu - s) + sigma n)`` in float64, then ``action = float32(float64(action) + s)``.  The normals come from
    the query's Philox streams keyed by the GLOBAL env id, so a split batch reproduces the whole one; torch's generator plays no part.
    ``reset(mask)`` puts the masked envs (all of them without a mask) back to ``mu``; like the reference's, ``rollout`` never resets it."""

    def __init__(self, num_envs: int, action_dim: int, mu: float = 0.0, theta: float = 0.3, sigma: float = 0.05, device=None):
        import torch

        num_envs, action_dim = int(num_envs), int(action_dim)
        if num_envs < 1 or action_dim < 1:
            raise ValueError(f"DeviceOUNoise: num_envs ({num_envs}) and action_dim ({action_dim}) must be >= 1")
        self.mu, self.theta, self.sigma = float(mu), float(theta), float(sigma)
        if not all(math.isfinite(v) for v in (self.mu, self.theta, self.sigma)) or self.sigma < 0:
            raise ValueError(f"DeviceOUNoise: mu, theta, sigma must be finite and sigma >= 0 (got {self.mu}, {self.theta}, {self.sigma})")
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise ValueError(f"DeviceOUNoise: the state lives on the GPU, not on {device}")
        self.state = torch.full((num_envs, action_dim), self.mu, dtype=torch.float64, device=device)

    def reset(self, mask=None):
        import torch

        if mask is None:
            self.state.fill_(self.mu)
            return
        m = torch.as_tensor(mask, device=self.state.device)
        if m.dtype != torch.bool or tuple(m.shape) != (self.state.shape[0],):
            raise ValueError(f"DeviceOUNoise.reset: mask must be a bool vector of {self.state.shape[0]} entries")
        self.state[m] = self.mu

    def get_state(self):
        """A copy of the float64 state [num_envs, action_dim]: with ``DeviceActor.get_state`` and the env's, what a checkpoint of an
        exploring rollout holds."""
        return self.state.clone()

    def set_state(self, state):
        """Resume from ``get_state`` (in place: queries already hold the tensor's address).  ValueError for another shape."""
        import torch

        st = torch.as_tensor(state, device=self.state.device)
        if tuple(st.shape) != tuple(self.state.shape):
            raise ValueError(f"DeviceOUNoise.set_state: the state is {tuple(st.shape)}, this process {tuple(self.state.shape)}")
        self.state.copy_(st.to(torch.float64))

    def check(self, batch: int, action_dim: int, device):
        """ValueError unless the state fits a query of ``batch`` rows and ``action_dim`` units on ``device``."""
        import torch

        st = self.state
        if (not isinstance(st, torch.Tensor) or st.dtype != torch.float64 or not st.is_contiguous() or tuple(st.shape) != (int(batch), int(action_dim))
                or st.device != torch.device(device)):
            raise ValueError(f"ou_noise: the state must be a contiguous float64 [{batch}, {action_dim}] tensor on {device} "
                             f"(got {getattr(st, 'dtype', type(st))} {tuple(getattr(st, 'shape', ()))} on {getattr(st, 'device', None)})")


def action_noise(ou_noise=None, action_mode: str = "sample"):
    """The ``aog_action_noise`` of a HIP query, or None when both are the defaults (the plain entry points run).  ValueError for an unknown
    mode or an ``ou_noise`` that is not a ``DeviceOUNoise``."""
    from . import _lib

    if action_mode not in _lib.AOG_ACTION_MODE:
        raise ValueError(f"action_mode must be 'sample' or 'mean' (got {action_mode!r})")
    if ou_noise is not None and not isinstance(ou_noise, DeviceOUNoise):
        raise ValueError("ou_noise of a HIP policy query must be a DeviceOUNoise (the torch OrnsteinUhlenbeckNoise is added outside the query)")
    if ou_noise is None and action_mode == "sample":
        return None
    ptr, mu, theta, sigma = (None, 0.0, 0.0, 0.0) if ou_noise is None else (ou_noise.state.data_ptr(), ou_noise.mu, ou_noise.theta, ou_noise.sigma)
    return _lib.AogActionNoise(_lib.AOG_ACTION_MODE[action_mode], 0, ptr, mu, theta, sigma)


# rollout()'s DeviceActor per actor module.  Kept here, NOT on the module: a DeviceActor holds the ctypes library handle, which can be
# neither deep-copied (target networks) nor pickled (torch.save of the module).  Weak keys, and DeviceActor only holds a weak
# reference back to its module, so neither keeps the other alive.
_DEVICE_ACTORS = weakref.WeakKeyDictionary()


class DeviceActor:
    """The policy query (``Actor.forward`` + ``get_action``, network.py:48-69) as ONE library launch (``aog_actor_act``): the
    weights of a torch module built by ``make_actor`` or of the reference's own ``Actor`` (``actor_layers``: recognised by attribute name)
    are read in place on every call, so a learner may keep updating them.  Dropout masks / Gaussian noise come from the
    library's Philox streams keyed by (seed, call counter, GLOBAL env id, layer, unit), not from torch's generator.  Keep ONE
    instance alive for the whole training run: its call counter is what makes every query draw fresh masks and noise
    (``rollout`` caches it per actor module for that reason).  ``env_id_base`` = global id of obs row 0 (multi-GPU: the
    env's ``global_env_offset``), so ranks explore with independent noise and a split batch reproduces the unsplit one."""

    def __init__(self, actor, seed: int = 0, dropout_p: float = 0.5, env_id_base: int = 0):
        import ctypes as C

        from . import _lib

        self._C, self._lib_mod = C, _lib
        if actor_layers(actor) is None:
            raise ValueError("DeviceActor: the module exposes neither layer1a / layer2a / layer3a / outputa (the reference's Actor, network.py:17-39) "
                             "nor hidden (3 x nn.Linear) + out")
        self.lib = _lib.load()
        self._actor_ref = weakref.ref(actor)
        self.seed = int(seed)
        self.dropout_p = float(dropout_p)
        self.env_id_base = int(env_id_base)
        self.calls = 0

    @property
    def actor(self):
        a = self._actor_ref()
        if a is None:
            raise RuntimeError("DeviceActor: the actor module it was built for has been garbage-collected")
        return a

    def get_state(self):
        """What keys the query's random streams besides the env ids: {"seed", "calls", "env_id_base", "dropout_p"}.  The env's ``get_state`` does
        not hold it (the policy is not the env's); a checkpoint of an exploring rollout saves both (and the weights, which are torch's)."""
        return {"seed": self.seed, "calls": self.calls, "env_id_base": self.env_id_base, "dropout_p": self.dropout_p}

    def set_state(self, state):
        """Resume from ``get_state``: the next query draws what the saved instance's next query would have drawn.  ValueError when the
        state was saved for another ``env_id_base`` (another slice of the batch)."""
        if int(state["env_id_base"]) != self.env_id_base:
            raise ValueError(f"DeviceActor.set_state: the state was saved at env_id_base {state['env_id_base']}, this instance serves {self.env_id_base}")
        self.seed, self.calls, self.dropout_p = int(state["seed"]), int(state["calls"]), float(state["dropout_p"])

    def layers(self):
        """The four ``nn.Linear`` of the module, checked: contiguous float32 CUDA weights (ValueError otherwise)."""
        import torch

        layers = actor_layers(self.actor)
        for layer in layers:
            if layer.weight.dtype != torch.float32 or not layer.weight.is_contiguous() or not layer.weight.is_cuda:
                raise ValueError("DeviceActor needs contiguous float32 CUDA weights")
        return layers

    def net(self, batch: int, cov_var: float = 0.5, layers=None):
        """The ``aog_actor`` of the NEXT query (call index ``self.calls``) for ``batch`` observation rows.  Does not advance the counter: a
        caller whose launch makes the query (``__call__``, ``BatchedAOEnv.step_with_policy``) adds one, so every query draws fresh streams."""
        layers = self.layers() if layers is None else layers
        S, H, A = layers[0].weight.shape[1], layers[0].weight.shape[0], layers[3].weight.shape[0]
        C, _lib = self._C, self._lib_mod
        return _lib.AogActor(int(batch), S, H, A, self.env_id_base, 0, *[C.c_void_p(t.data_ptr()) for layer in layers for t in (layer.weight, layer.bias)],
                             self.dropout_p, float(cov_var), self.seed, self.calls)

    def __call__(self, obs, cov_var: float = 0.5, out=None, ou_noise=None, action_mode: str = "sample"):
        """obs [B, S] float16 or float32 on the GPU -> (action [B, A] float32, log_prob [B] float32, mean [B, A]).  ``action_mode="mean"``:
        the action is the mean (dropout still active) and log_prob the density there; ``ou_noise`` (a ``DeviceOUNoise`` of [B, A]): its
        state advances once and is added to the action (``aog_actor_act_noise``)."""
        import torch

        C, _lib = self._C, self._lib_mod
        layers = self.layers()
        if obs.dtype not in (torch.float16, torch.float32) or not obs.is_contiguous():
            raise ValueError("obs must be a contiguous float16 or float32 tensor")
        B, S = obs.shape
        H, A = layers[0].weight.shape[0], layers[3].weight.shape[0]
        if layers[0].weight.shape[1] != S:
            raise ValueError("obs width does not match the actor's first layer")
        if out is None:
            action = torch.empty((B, A), dtype=torch.float32, device=obs.device)
            log_prob = torch.empty((B,), dtype=torch.float32, device=obs.device)
            mean = torch.empty((B, A), dtype=torch.float32, device=obs.device)
        else:
            action, log_prob, mean = out
        noise = action_noise(ou_noise, action_mode)
        if ou_noise is not None:
            ou_noise.check(B, A, obs.device)
        net = self.net(B, cov_var, layers)
        self.calls += 1
        args = (C.byref(net), obs.device.index or 0, C.c_void_p(obs.data_ptr()), int(obs.dtype == torch.float16), C.c_void_p(mean.data_ptr()),
                C.c_void_p(action.data_ptr()), C.c_void_p(log_prob.data_ptr()))
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if noise is None:
            _lib.check(self.lib.aog_actor_act(*args, stream))
        else:
            _lib.check(self.lib.aog_actor_act_noise(*args, C.byref(noise), stream))
        return action, log_prob, mean


# One row of rollout's policy table.  noun: what the messages call the source of the action; act(env, ctrl, row, first): writes the step's
# [B, A] action into ``row`` (None: the policy query); sh: needs an env built with SH_operation=True, the action being a controller's raw
# actuator vector; pyramid: needs env.pyramid; keyword: the rollout keyword that carries its controller (``ctrl``); refuses: reason -> the
# options it refuses for that reason (keys of ``given`` in rollout), the reasons being checked in the order of _REFUSALS; fused: which of the
# env's fused forms runs it under fused_policy=True ("policy": reset_with_policy / step_with_policy, "spgd": reset_with_spgd / step_with_spgd)
_NOT_A_QUERY = {"query": ("dev_ou", "mean"), "fused": ("fused_policy",)}
_MEASURES = {"query": ("dev_ou", "mean"), "measurement": ("lookahead", "fused_policy")}
_Policy = namedtuple("_Policy", "noun act sh pyramid keyword refuses fused", defaults=(None, True, False, None, _NOT_A_QUERY, None))

# the message of each reason for refusing an option, in the order they are checked (the env's own conditions come after "query")
_REFUSALS = {
    "experiment": "policy='spgd' goes with none of lookahead, science, ou_noise and action_mode='mean': the controller's commands are the "
                  "experiment (a noise term or another mirror command between two of its queries would enter its metric differences)",
    "query": "policy={policy!r} takes neither a DeviceOUNoise nor action_mode='mean' (the {noun} is not a policy query)",
    "measurement": "policy={policy!r} goes with neither lookahead nor fused_policy: its measurement is refused while the next screens or "
                   "the next action are already in place",
    "fused": "fused_policy=True needs policy='actor' (neither the Shack-Hartmann integrator nor the ideal controller is a policy query)",
}
_POLICIES = {
    "actor": _Policy("policy query", sh=False, refuses={}, fused="policy"),
    "shack": _Policy("Shack-Hartmann integrator", lambda env, ctrl, row, first: row.copy_(env.SH_step()[0])),
    "ideal": _Policy("ideal modal controller", lambda env, ctrl, row, first: row.copy_(env.ideal_action())),
    "pyramid": _Policy("pyramid integrator", lambda env, ctrl, row, first: row.copy_(env.PYR_step()[0]), pyramid=True),
    "predictive": _Policy("predictive controller", lambda env, ctrl, row, first: row.copy_(ctrl.action()), keyword="predictor", refuses=_MEASURES),
    "modal": _Policy("modal integrator", lambda env, ctrl, row, first: row.copy_(ctrl.action()), keyword="controller", refuses=_MEASURES),
    "lqg": _Policy("LQG controller", lambda env, ctrl, row, first: row.copy_(ctrl.action()), keyword="controller", refuses=_MEASURES),
    # (the controller is reset with the env; every later step queries it on the last step's metric)
    "spgd": _Policy("SPGD controller", lambda env, ctrl, row, first: ctrl.reset(out=row) if first else ctrl.action(out=row), keyword="controller",
                    refuses={"experiment": ("lookahead", "science", "ou_noise", "mean")}, fused="spgd"),
    # (the integrator assumes the mirrors hold its command: where episodes start with flat mirrors it starts at zero with them)
    "tomographic": _Policy("tomographic controller", lambda env, ctrl, row, first: (
        ctrl.reset() if first and getattr(env, "flat_mirror_start_per_episode", False) else None, ctrl.action(out=row))[1], keyword="controller",
                           refuses=_MEASURES),
}
_CONTROLLER_KEYWORDS = {
    "predictor": "policy='predictive' takes its controller as predictor=PredictiveController(env, ...), and no other policy takes one",
    "controller": "policy='modal' takes its controller as controller=ModalIntegrator(env, ...), policy='lqg' as "
                  "controller=LQGController(env, ...), policy='spgd' as controller=SPGDController(env, ...), policy='tomographic' as "
                  "controller=TomographicController(env, ...), and no other policy takes one",
}


def _transition_buffers(n, B, S, A, obs_dtype, dev):
    """rollout's six ``[n = T*E, B, ...]`` tensors, written in place, and one spare ``[B, A]`` float32 row (the policy query's mean; the
    command the last step of a fused SPGD episode does not write)."""
    import torch

    def rows(*shape, dtype=torch.float32):
        return torch.empty((n, B) + shape, dtype=dtype, device=dev)

    return ({"obs": rows(S, dtype=obs_dtype), "act": rows(A), "log_prob": rows(), "rew": rows(), "next_obs": rows(S, dtype=obs_dtype),
             "done": rows(dtype=torch.bool)}, torch.empty((B, A), dtype=torch.float32, device=dev))


def _run_episodes(T, episodes, gatherer, reset, step):
    """rollout's episode skeleton.  ``reset(i0)`` -> (the buffers, the reset observation): starts an episode whose rows begin at ``i0``
    (the buffers may be made at the first call, once the shapes are known); ``step(i, t, obs)`` -> the next observation (None where the
    form has no use for it): step ``t`` of the episode, which fills ``act`` / ``log_prob`` (unless the form did so earlier) and ``next_obs`` / ``rew`` / ``done`` of row ``i``.
    All envs run in lock-step: ``done`` is identical for every env (AO_env.py:147), so no host sync is needed to end an episode."""
    ep_returns = []
    for e in range(episodes):
        i0 = e * T
        out, obs = reset(i0)
        gatherer.start_episode()
        out["obs"][i0].copy_(obs)
        for t in range(T):
            obs = step(i0 + t, t, obs)
        if T > 1:
            out["obs"][i0 + 1:i0 + T].copy_(out["next_obs"][i0:i0 + T - 1])   # obs of step t+1 = next_obs of step t
        gatherer.add(out["rew"][i0:i0 + T].sum(0))
        ep_returns.append(gatherer.finish_episode().clone())
    return out, ep_returns


def _out_of_step(who, what, queried, t, T):
    return RuntimeError(f"{who} {'did not query' if queried is None else 'queried'} the {what} at step {t + 1} of {T}: the env's "
                        "episode length differs from timesteps_per_episode")


def rollout(env, actor, episodes: int = 1, cov_var: float = 0.5, gatherer=None, generator=None, actor_impl: str = "auto", seed: int = 0,
            dev_actor=None, lookahead: bool = False, policy: str = "actor", ou_noise=None, fused_policy: bool = False, action_mode: str = "sample",
            science: bool = False, predictor=None, controller=None, link=None):
    """Collect ``episodes`` lock-step episodes from ``env`` (a ``BatchedAOEnv``).

    Returns a dict of device tensors shaped ``[T*E, B, ...]`` (obs, act, log_prob, rew, next_obs, done), ``ep_returns`` ``[E, B_global]``
    (gathered over ranks when ``gatherer`` is distributed), ``avg_ep_rew`` (the reference's logged scalar) and ``batch_lens``
    (``algorithm.py:226,283``: a numpy array of T*E zeros whose first E entries hold the length of each episode — always T here: ``done``
    depends on the step counter only).  Every condition below is checked before anything runs: ValueError.

    ``policy="actor"``: the action is the policy query on the last observation.  ``actor_impl``: "hip" = the fused policy-query kernel
    (``DeviceActor``), "torch" = the module's own forward + ``sample_action``, "auto" = "hip" for CUDA modules with the ``make_actor``
    structure.  The ``DeviceActor`` (and with it the call counter of its random streams) persists across calls: pass one in as ``dev_actor``,
    or let this function cache it (in a module-level weak dictionary keyed by the actor: the caller's module stays deep-copyable and
    picklable) — a training loop that calls ``rollout`` once per iteration (algorithm.py:156) then explores with fresh dropout masks and
    noise in every iteration, like the reference's torch generator does.

    The other policies take no query: the action is a controller's raw actuator vector, so they need an env built with
    ``SH_operation=True``, ``actor`` may be None, ``log_prob`` holds the reference's constant 1, and they take neither a ``DeviceOUNoise``
    nor ``action_mode="mean"``.

    ``policy="shack"`` (``algorithm.py:252-253``, the 'SHACK' algorithm): ``env.SH_step()``, the Shack-Hartmann integrator on the device.

    ``policy="ideal"``: the ideal modal controller — ``env.ideal_action()``, the best-fit mirror command of the state the last
    observation saw, applied to the next screen (the one-frame lag every controller has): the ceiling Shack-Hartmann and learnt policies
    are read against.

    ``policy="pyramid"``: ``env.PYR_step()[0]``, the modulated pyramid sensor's integrator (an env built with ``pyramid=dict(...)``).

    ``policy="predictive"``: ``predictor.action()`` of the ``predictor.PredictiveController`` passed as ``predictor`` (built for this env):
    a linear predictor of the next best-fit command, learnt on the device by recursive least squares from the measurements the loop
    takes — what recovers the one-frame lag ``"ideal"`` commits.  The predictor is NOT reset at episode ends (the atmosphere is not reset
    either); not with ``lookahead`` or ``fused_policy``.

    ``policy="modal"``: ``controller.action()`` of the ``telemetry.ModalIntegrator`` passed as ``controller`` (built for this env): the
    integrator with one gain per (env, mode), which also records the measurements it takes (``controller.retune()`` then sets the
    optimised modal gains).  Same conditions as ``"predictive"``; neither its command nor its telemetry is reset at episode ends.

    ``policy="lqg"``: ``controller.action()`` of the ``lqg.LQGController`` passed as ``controller`` (built for this env): per mode a Kalman
    filter on a turbulence-plus-vibration model that predicts the measurement ``delay`` frames ahead, which also records the measurements it
    takes (``controller.identify()`` then refits the turbulence).  Same conditions as ``"predictive"``; neither its filter nor its
    telemetry is reset at episode ends.

    ``policy="spgd"``: the sensorless baseline — the ``sensorless.SPGDController`` passed as ``controller`` (built for this env), which
    sees only the scalar metric of the last step; it is reset with the env at every episode start (all envs; its iteration counters go
    on).  Not with ``lookahead``, ``science``, ``ou_noise`` or ``action_mode="mean"``.  With ``fused_policy=True`` it goes through
    ``env.reset_with_spgd`` / ``env.step_with_spgd`` (the query rides in the step's last launch) and returns the same dict, bit for bit, as
    the unfused loop from the same controller state.

    ``policy="tomographic"``: ``controller.action()`` of the ``tomography.TomographicController`` passed as ``controller`` (built for this
    env, a ``LayeredAOEnv`` with ``altitude_mirrors``): the multi-conjugate baseline — it measures on its guide directions, sets the altitude
    mirrors' commands itself and returns the pupil mirror's actuators, which are the stored action.  Reset with the env at every episode
    start when episodes start with flat mirrors.  Same conditions as ``"predictive"``; with sightlines attached the loop is the unfused one.

    ``ou_noise`` (``algorithm.py:258-259``, DDPG): an ``OrnsteinUhlenbeckNoise`` whose sample is added to every action before the env sees
    it (and before it is stored, like the reference's in-place ``action +=``), or a ``DeviceOUNoise`` (``main.py:218-220``: mu 0, theta
    0.3, sigma 0.05), which the HIP policy query advances and adds itself: float64 state, Philox normals keyed by the global env id (a
    split batch reproduces the whole one), no extra launch; it needs the HIP query.  Neither is reset here, as in the reference.

    ``action_mode="mean"`` (evaluation, ``eval_policy.py:31``): the action is the policy's mean with dropout still active, ``log_prob`` the
    density of ``N(mean, cov_var I)`` there; with ``actor_impl="torch"`` the action is ``actor(obs)``.

    ``fused_policy=True``: the policy query rides with the env step (``env.reset_with_policy`` / ``env.step_with_policy``, one launch where
    the epilogue of step t, the query on its observation and the prologue of step t + 1 take three): needs ``policy="actor"`` resolved to
    ``actor_impl="hip"`` (or ``policy="spgd"``, above), and takes a ``DeviceOUNoise`` and ``action_mode`` but not the torch
    ``OrnsteinUhlenbeckNoise`` (that noise would have to be added between the query and the prologue).  Returns the same dict, bit for
    bit, as the unfused loop with the same ``DeviceActor`` (seed and call counter) and, if any, an OU state equal to the unfused loop's.
    Not for an env built with ``servo=``: its steps go through ``env.step``, the unfused loop, where the servo sits between the stored action
    (the command, ``out["act"]``) and the mirror.

    ``lookahead=True`` (dynamic atmosphere on the device stream): the next step's wind extrusion is launched on the library's own stream
    beside this step's epilogue and the policy query — bit-identical results; the screens are off limits between two steps of an
    episode, which this loop never touches.  Off by default: on ROCm 7.2 the two cross-stream event hand-offs it needs cost what the
    overlap saves.

    ``science=True`` (an env built with ``science_window``): ``env.science_integrate()`` after every step, never cleared here — read the
    long exposure with ``env.science_exposure()`` afterwards.  The transitions are those of ``science=False`` bit for bit.  Not with
    ``fused_policy`` or ``lookahead`` (the camera is refused while the next action or the next screens are already in place).

    ``link`` (a ``link.LinkTelemetry`` built for the env's ``num_envs`` and device): ``link.push(info["power"])`` after every step of every
    policy, the fused and look-ahead forms included; never reset here — read ``link.statistics()`` afterwards.  The transitions are those
    of ``link=None`` bit for bit.  An env with ``scintillation`` pushes ``info["scintillation"]["power"]`` instead (the power with the
    log-amplitude on the pupil) and runs the unfused loop only."""
    import inspect

    import numpy as np
    import torch

    from .sharding import EpisodeReturnGatherer

    T = int(env.max_steps)
    B = env.num_envs
    if gatherer is None:
        gatherer = EpisodeReturnGatherer(B, env.device, False)
    if fused_policy and getattr(env, "servo", None) is not None:
        raise ValueError("fused_policy=True: this env has a mirror servo attached, and the fused forms load the action inside the step's launch, "
                         "where the servo has no place — the unfused loop (fused_policy=False) steps through it")
    if fused_policy and getattr(env, "scintillation_on", False):
        raise ValueError("fused_policy=True: this env has scintillation on, and its receiver reads the mirror between two steps, where a fused step "
                         "already holds the next action — the unfused loop (fused_policy=False) steps through it")
    if policy not in _POLICIES:
        raise ValueError("policy must be 'actor', 'shack', 'ideal', 'pyramid', 'predictive', 'modal', 'lqg', 'spgd' or 'tomographic'")
    if action_mode not in ("sample", "mean"):
        raise ValueError(f"action_mode must be 'sample' or 'mean' (got {action_mode!r})")
    pol, ctrl = _POLICIES[policy], None
    for keyword, message in _CONTROLLER_KEYWORDS.items():
        passed = predictor if keyword == "predictor" else controller
        if (pol.keyword == keyword) != (passed is not None):
            raise ValueError(message)
        if pol.keyword == keyword:
            if passed.env is not env:
                raise ValueError(f"policy={policy!r}: the {keyword} was built for another env")
            ctrl = passed
    dev_ou = isinstance(ou_noise, DeviceOUNoise)
    given = {"lookahead": lookahead, "fused_policy": fused_policy, "science": science, "ou_noise": ou_noise is not None, "dev_ou": dev_ou,
             "mean": action_mode != "sample"}

    def refuse(reason):
        if any(given[option] for option in pol.refuses.get(reason, ())):
            raise ValueError(_REFUSALS[reason].format(policy=policy, noun=pol.noun))

    refuse("experiment")
    refuse("query")
    if pol.sh:
        if not getattr(env, "SH_operation", False):
            raise ValueError(f"policy={policy!r} needs an env created with SH_operation=True (AO_env.py:115-116, 254)")
        if pol.pyramid and getattr(env, "pyramid", None) is None:
            raise ValueError("policy='pyramid' needs an env created with pyramid=dict(...)")
        refuse("measurement")
        actor_impl = "none"
    elif actor_impl == "auto":
        actor_impl = "hip" if actor_layers(actor) is not None and next(actor.parameters()).is_cuda else "torch"
    if actor_impl != "hip":
        dev_actor = None
    elif dev_actor is None:
        base = int(getattr(env, "global_env_offset", 0))
        dev_actor = _DEVICE_ACTORS.get(actor)
        if dev_actor is None or dev_actor.seed != int(seed) or dev_actor.env_id_base != base or dev_actor.actor is not actor:
            dev_actor = DeviceActor(actor, seed=seed, env_id_base=base)
            _DEVICE_ACTORS[actor] = dev_actor
    if dev_ou and not pol.sh and dev_actor is None:
        raise ValueError("a DeviceOUNoise is advanced by the HIP policy query (actor_impl='hip'); the torch query takes an OrnsteinUhlenbeckNoise")
    # the query's action-form keywords, passed only when they differ from the defaults
    pkw = {}
    if dev_ou:
        pkw["ou_noise"] = ou_noise
    if action_mode != "sample":
        pkw["action_mode"] = action_mode
    refuse("fused")
    if fused_policy and not pol.sh:
        if dev_actor is None:
            raise ValueError("fused_policy=True needs the HIP policy query (actor_impl='hip': a make_actor / reference Actor module with CUDA weights)")
        if ou_noise is not None and not dev_ou:
            raise ValueError("fused_policy=True cannot add the torch ou_noise: the noise would have to enter between the policy query and the "
                             "prologue (a DeviceOUNoise is added inside the query)")
    if science:
        if getattr(env, "science_window", None) is None:
            raise ValueError("science=True needs an env created with science_window=...")
        if fused_policy or lookahead:
            raise ValueError("science=True goes with neither fused_policy nor lookahead: between two such steps the mirror or the screens already "
                             "belong to the next step and the camera is refused")
    if link is not None:
        from .link import check_link

        check_link(link, env)
    step_takes_out = "out" in inspect.signature(env.step).parameters
    scintillating = bool(getattr(env, "scintillation_on", False))
    looking_ahead = bool(env.lookahead(True)) if (lookahead and callable(getattr(env, "lookahead", None))) else False
    n = T * episodes
    out = spare = None

    def buffers(S, A, obs_dtype, dev):
        nonlocal out, spare
        out, spare = _transition_buffers(n, B, S, A, obs_dtype, dev)
        if pol.sh:
            out["log_prob"].fill_(1.0)   # the reference's constant log-probability 1

    if fused_policy:
        # the env's reset writes row i0's action, step i the action of row i + 1 (none on the last step: the spare row stands in)
        buffers(int(env.obs_dim) ** 2, int(env.num_modes), torch.float16, env.device)
        act, logp, nobs, rew, done = (out[k] for k in ("act", "log_prob", "next_obs", "rew", "done"))
        end = T - 1
        if pol.fused == "spgd":
            def reset(i0):
                return out, env.reset_with_spgd(ctrl, action_out=act[i0])[0][0]

            def step(i, t, obs):
                ret, nxt = env.step_with_spgd(ctrl, out=(nobs[i], rew[i], done[i]), action_out=spare if t == end else act[i + 1])
                if (nxt is None) != (t == end):
                    raise _out_of_step("step_with_spgd", "controller", nxt, t, T)
                if link is not None:
                    link.push(ret[4]["power"])
        else:
            def reset(i0):
                return out, env.reset_with_policy(dev_actor, cov_var, policy_out=(act[i0], logp[i0], spare), **pkw)[0][0]

            def step(i, t, obs):
                ret, nxt = env.step_with_policy(dev_actor, cov_var, out=(nobs[i], rew[i], done[i]),
                                                policy_out=None if t == end else (act[i + 1], logp[i + 1], spare), **pkw)
                if (nxt is None) != (t == end):
                    raise _out_of_step("step_with_policy", "policy", nxt, t, T)
                if link is not None:
                    link.push(ret[4]["power"])
    else:
        def reset(i0):
            obs = env.reset()[0]
            if out is None:   # the buffers are laid out once the shapes are known
                A = int(env.num_modes) if pol.sh else int(list(actor.parameters())[-1].shape[0])   # width of the output layer's bias
                buffers(obs.shape[1], A, obs.dtype, obs.device)
            return out, obs

        def step(i, t, obs):
            action = row = out["act"][i]   # (action: what the env is handed)
            log_prob = out["log_prob"][i]
            if pol.sh:
                pol.act(env, ctrl, row, t == 0)
            elif dev_actor is not None:
                dev_actor(obs, cov_var, out=(row, log_prob, spare), **pkw)
            elif action_mode == "mean":   # eval_policy.py:31: the mean, dropout still active; log_prob = the density at the mean
                row.copy_(actor(obs))
                log_prob.fill_(-0.5 * row.shape[-1] * math.log(2 * math.pi * cov_var))
            else:
                action, lp = sample_action(actor(obs), cov_var, generator)
                row.copy_(action)
                log_prob.copy_(lp)
            if ou_noise is not None and not dev_ou:
                row.add_(ou_noise.sample())           # algorithm.py:258-259
                action = row
            transition = (out["next_obs"][i], out["rew"][i], out["done"][i])
            if step_takes_out:   # the env writes the transition straight into this step's slices
                next_obs, _, _, _, info = env.step(action, out=transition)
            else:
                next_obs, rew, done, _, info = env.step(action)
                for dst, src in zip(transition, (next_obs, rew, done)):
                    dst.copy_(src)
            if science:
                env.science_integrate()
            if link is not None and scintillating:   # (behind the option: the power the amplitude-aware receiver couples)
                link.push(info["scintillation"]["power"].to(torch.float32))
            elif link is not None:
                link.push(info["power"])
            return next_obs

    with torch.no_grad():
        out, ep_returns = _run_episodes(T, episodes, gatherer, reset, step)
    if looking_ahead:
        env.lookahead(False)
    out["ep_returns"] = torch.stack(ep_returns)
    out["avg_ep_rew"] = float(out["ep_returns"].mean().item()) / T
    lens = np.zeros(n)
    lens[:episodes] = T
    out["batch_lens"] = lens
    return out


def replay_transitions(batch, episode_major: bool = False):
    """The hand-off to a replay buffer (``ReplayBuffer.add(state, action, reward, next_state, done)``, ``replay_buffer.py:21-25``;
    ``sample_batch`` stacks exactly these five, ``:30-34``): the ``[T*E, B, ...]`` tensors of ``rollout`` as five flat device tensors
    ``(state [n, o*o], action [n, A], reward [n], next_state [n, o*o], done [n])``, n = T*E*B.

    Order: step-major (all envs of step 0, then step 1, ...) — the order a vectorised collector appends in; ``episode_major=True``
    gives env-major order instead (each env's steps contiguous: the order ``B`` single-env collectors appending one after the other
    would produce, ``algorithm.py:238-276``).  Views where the layout allows, no host copy."""
    keys = ("obs", "act", "rew", "next_obs", "done")
    out = []
    for k in keys:
        t = batch[k]
        if episode_major:
            t = t.transpose(0, 1)
        out.append(t.reshape((t.shape[0] * t.shape[1],) + tuple(t.shape[2:])))
    return tuple(out)
