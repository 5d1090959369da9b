"""Host logic of rollout(fused_policy=True) (no GPU): a stand-in env with the reset_with_policy / step_with_policy interface and a stand-in
policy in place of DeviceActor, both on CPU tensors."""
import numpy as np
import pytest
import torch

from adaptive_optics_gym_amd.rollout import OrnsteinUhlenbeckNoise, make_actor, rollout


class FakePolicy:
    """Deterministic in (obs, call index), like DeviceActor's Philox streams."""

    def __init__(self):
        self.calls, self.env_id_base = 0, 0

    def query(self, obs, out):
        action, log_prob, mean = out
        base = obs.float().mean(dim=1, keepdim=True)
        mean.copy_(base + torch.arange(mean.shape[1], dtype=torch.float32))
        action.copy_(mean + 0.25 * self.calls)
        log_prob.copy_(base[:, 0] - self.calls)
        self.calls += 1
        return action, log_prob, mean

    def __call__(self, obs, cov_var=0.5, out=None):
        return self.query(obs, out)


class FakeEnv:
    def __init__(self, B, o, A, T):
        self.num_envs, self.max_steps, self.device = B, T, torch.device("cpu")
        self.obs_dim, self.num_modes, self.t = o, A, 0
        self.stepped = []   # the actions each step used, in order
        self.pending = None
        self.queries = []   # (kind, step index) of every fused policy query

    def _obs(self):
        return torch.full((self.num_envs, self.obs_dim ** 2), float(self.t), dtype=torch.float16) + torch.arange(self.num_envs)[:, None].half()

    def reset(self):
        assert self.pending is None
        self.t = 0
        return self._obs(), {}

    def step(self, a, out=None):
        assert self.pending is None
        self.t += 1
        self.stepped.append(a.clone())
        rew = -a.abs().mean(dim=1) - self.t
        done = torch.full((self.num_envs,), self.t == self.max_steps)
        obs = self._obs()
        if out is not None:
            out[0].copy_(obs)
            out[1].copy_(rew)
            out[2].copy_(done)
            obs, rew, done = out
        return obs, rew, done, torch.zeros(self.num_envs, dtype=torch.bool), {}

    def reset_with_policy(self, policy, cov_var=0.5, policy_out=None):
        obs, info = self.reset()
        pol = policy.query(obs, policy_out)
        self.pending = pol[0]
        self.queries.append(("reset", 0))
        return (obs, info), pol

    def step_with_policy(self, policy, cov_var=0.5, out=None, policy_out=None, action=None):
        assert (action is None) == (self.pending is not None)
        a = self.pending if action is None else action
        self.pending = None
        ret = self.step(a, out=out)
        if self.t == self.max_steps:
            return ret, None
        pol = policy.query(ret[0], policy_out)
        self.pending = pol[0]
        self.queries.append(("step", self.t))
        return ret, pol


def _both(B=3, o=2, A=5, T=4, E=2):
    outs, envs, pols = [], [], []
    for fused in (False, True):
        env, pol = FakeEnv(B, o, A, T), FakePolicy()
        actor = make_actor(o * o, A, 8)   # (the unfused loop reads the action width off the module; the stand-in policy acts)
        outs.append(rollout(env, actor, episodes=E, actor_impl="hip", dev_actor=pol, fused_policy=fused))
        envs.append(env)
        pols.append(pol)
    return outs, envs, pols


def test_fused_rows_match_unfused_loop():
    (ref, got), (env_ref, env_got), (pol_ref, pol_got) = _both()
    for k in ("obs", "act", "log_prob", "rew", "next_obs", "done", "ep_returns"):
        assert torch.equal(ref[k], got[k]), k
    assert pol_ref.calls == pol_got.calls == 8
    assert all(torch.equal(a, b) for a, b in zip(env_ref.stepped, env_got.stepped))
    np.testing.assert_array_equal(ref["batch_lens"], got["batch_lens"])
    assert ref["avg_ep_rew"] == got["avg_ep_rew"]


def test_fused_row_bookkeeping():
    B, T, E = 3, 4, 2
    (_, got), (_, env), _ = _both(B=B, T=T, E=E)
    # reset fills row i0, step i fills row i + 1, the episode's last step queries nothing
    assert env.queries == [("reset", 0), ("step", 1), ("step", 2), ("step", 3)] * E
    for i, a in enumerate(env.stepped):
        assert torch.equal(got["act"][i], a)   # row i holds the action step i stepped
    assert torch.equal(got["obs"][1:T], got["next_obs"][0:T - 1])
    assert torch.equal(got["obs"][T], torch.arange(B)[:, None].half().expand(B, 4))   # the second episode's reset observation
    lens = np.zeros(T * E)
    lens[:E] = T
    np.testing.assert_array_equal(got["batch_lens"], lens)
    ep = got["rew"].reshape(E, T, B).sum(1)
    assert abs(got["avg_ep_rew"] - float(ep.mean()) / T) < 1e-6


def test_fused_policy_refusals():
    env = FakeEnv(2, 2, 4, 3)
    with pytest.raises(ValueError, match="ou_noise"):
        rollout(env, None, actor_impl="hip", dev_actor=FakePolicy(), fused_policy=True, ou_noise=OrnsteinUhlenbeckNoise(2, 4, 0.0, 0.15, 0.2))
    env.SH_operation = True
    with pytest.raises(ValueError, match="policy='actor'"):
        rollout(env, None, policy="shack", fused_policy=True)
    with pytest.raises(ValueError, match="actor_impl='hip'"):
        rollout(env, make_actor(4, 4, 8), actor_impl="torch", fused_policy=True)
    with pytest.raises(ValueError, match="actor_impl='hip'"):
        rollout(env, make_actor(4, 4, 8), fused_policy=True)   # "auto" resolves to the torch forward for a CPU module
    assert env.queries == [] and env.stepped == []
