"""Action forms of the policy query without a GPU: the C-ABI additions (aog_action_noise, the three _noise entry points), DeviceOUNoise's
checks and reset, rollout()'s new refusals, and which keywords reach the env and the query (stand-ins on CPU tensors)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.rollout import DeviceOUNoise, OrnsteinUhlenbeckNoise, action_noise, make_actor, rollout

AOG_ERR_INVALID = -1
NEW = ("aog_actor_act_noise", "aog_reset_act_noise", "aog_step_act_noise")


def _cpu_ou(B, A, mu=0.0, theta=0.3, sigma=0.05):
    """A DeviceOUNoise whose state sits on the CPU (its constructor insists on the GPU): for the host logic only, never given to the library."""
    ou = DeviceOUNoise.__new__(DeviceOUNoise)
    ou.mu, ou.theta, ou.sigma = mu, theta, sigma
    ou.state = torch.full((B, A), mu, dtype=torch.float64)
    return ou


def test_symbols_struct_and_abi(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "aog_action_noise" in header and re.search(r"#define AOG_ABI_VERSION\s+22\b", header)
    assert _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert lib.aog_abi_version() == 22
    assert C.sizeof(_lib.AogActionNoise) == 2 * 4 + 8 + 3 * 8
    assert lib.aog_struct_size(8) == C.sizeof(_lib.AogActionNoise)
    assert lib.aog_struct_size(9) == -1


def _fake_actor(batch):
    """An aog_actor whose (16-byte aligned, never dereferenced) weight pointers pass the host checks."""
    p = C.c_void_p(0x10000)
    return _lib.AogActor(batch, 4, 32, 16, 0, 0, *([p] * 8), 0.5, 0.5, 1, 0)


@pytest.mark.parametrize("field,value", [("mode", 2), ("mode", -1), ("reserved0", 1), ("ou_mu", math.nan), ("ou_theta", math.inf),
                                         ("ou_sigma", -math.inf), ("ou_sigma", -0.01), ("ou_sigma", math.nan)])
def test_bad_noise_is_invalid_before_any_device_work(field, value):
    lib = _lib.load()
    nz = _lib.AogActionNoise(0, 0, None, 0.0, 0.3, 0.05)
    setattr(nz, field, value)
    obs = C.c_void_p(0x20000)
    for batch in (0, 16):   # (batch 0 returns before any launch when the arguments are good)
        net = _fake_actor(batch)
        assert lib.aog_actor_act_noise(C.byref(net), 0, obs, 1, None, None, None, C.byref(nz), None) == AOG_ERR_INVALID
        assert b"aog_actor_act" in lib.aog_last_error()
    good = _lib.AogActionNoise(1, 0, None, 0.0, 0.3, 0.05)
    assert lib.aog_actor_act_noise(C.byref(_fake_actor(0)), 0, obs, 1, None, None, None, C.byref(good), None) == 0


def test_null_arguments_are_invalid():
    lib = _lib.load()
    nz = _lib.AogActionNoise(0, 0, None, 0.0, 0.3, 0.05)
    assert lib.aog_actor_act_noise(None, 0, C.c_void_p(0x20000), 1, None, None, None, C.byref(nz), None) == AOG_ERR_INVALID
    assert lib.aog_actor_act_noise(C.byref(_fake_actor(16)), 0, None, 1, None, None, None, None, None) == AOG_ERR_INVALID
    net = _fake_actor(16)
    assert lib.aog_reset_act_noise(None, C.byref(net), None, None, None, None, None, C.byref(nz), None) == AOG_ERR_INVALID
    queried = C.c_int(7)
    assert lib.aog_step_act_noise(None, C.byref(net), None, None, None, None, None, None, None, None, None, None, C.byref(queried), C.byref(nz),
                                  None) == AOG_ERR_INVALID
    assert queried.value == 0


def test_device_ou_noise_checks():
    for args in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            DeviceOUNoise(*args, device="cuda:0")
    for kw in (dict(mu=math.nan), dict(theta=math.inf), dict(sigma=-0.1), dict(sigma=math.nan)):
        with pytest.raises(ValueError):
            DeviceOUNoise(4, 4, device="cuda:0", **kw)
    with pytest.raises(ValueError):
        DeviceOUNoise(4, 4, device="cpu")
    ou = _cpu_ou(3, 2)
    ou.check(3, 2, "cpu")
    for B, A, dev in ((3, 3, "cpu"), (2, 2, "cpu"), (3, 2, "meta")):
        with pytest.raises(ValueError):
            ou.check(B, A, dev)
    ou.state = ou.state.float()
    with pytest.raises(ValueError):
        ou.check(3, 2, "cpu")
    ou.state = torch.zeros((2, 3), dtype=torch.float64).t()   # not contiguous
    with pytest.raises(ValueError):
        ou.check(3, 2, "cpu")


def test_device_ou_noise_reset_mask():
    ou = _cpu_ou(4, 3, mu=0.25)
    assert ou.state.dtype == torch.float64 and bool((ou.state == 0.25).all())
    ou.state.copy_(torch.arange(12, dtype=torch.float64).reshape(4, 3))
    ou.reset(torch.tensor([True, False, True, False]))
    assert ou.state[:, 0].tolist() == [0.25, 3.0, 0.25, 9.0]
    ou.reset([False, True, False, False])
    assert ou.state[1].tolist() == [0.25] * 3 and ou.state[3].tolist() == [9.0, 10.0, 11.0]
    for bad in (torch.tensor([1, 0, 1, 0]), torch.tensor([True, False])):
        with pytest.raises(ValueError):
            ou.reset(bad)
    ou.reset()
    assert bool((ou.state == 0.25).all())


def test_action_noise_struct():
    assert action_noise() is None
    nz = action_noise(None, "mean")
    assert (nz.mode, nz.reserved0, nz.ou_state) == (1, 0, None)
    ou = _cpu_ou(2, 2, mu=0.1, theta=0.3, sigma=0.05)
    nz = action_noise(ou)
    assert (nz.mode, nz.ou_state, nz.ou_mu, nz.ou_theta, nz.ou_sigma) == (0, ou.state.data_ptr(), 0.1, 0.3, 0.05)
    with pytest.raises(ValueError):
        action_noise(None, "greedy")
    with pytest.raises(ValueError):
        action_noise(OrnsteinUhlenbeckNoise(2, 2, 0.0, 0.3, 0.05))


class RecPolicy:
    """Stand-in for DeviceActor: records the keywords of every query; rejects the new ones unless told to accept them."""

    def __init__(self, accept):
        self.calls, self.env_id_base, self.accept, self.kws = 0, 0, accept, []

    def query(self, obs, out, kw):
        if kw and not self.accept:
            raise TypeError(f"unexpected keywords {sorted(kw)}")
        self.kws.append(dict(kw))
        action, log_prob, mean = out
        mean.copy_(obs.float().mean(dim=1, keepdim=True) + torch.arange(mean.shape[1], dtype=torch.float32))
        action.copy_(mean + 0.25 * self.calls)
        log_prob.fill_(-float(self.calls))
        self.calls += 1
        return action, log_prob, mean

    def __call__(self, obs, cov_var=0.5, out=None, **kw):
        return self.query(obs, out, kw)


class RecEnv:
    """Stand-in for BatchedAOEnv's fused interface: records the keywords of reset_with_policy / step_with_policy."""

    def __init__(self, B, o, A, T, accept):
        self.num_envs, self.max_steps, self.device = B, T, torch.device("cpu")
        self.obs_dim, self.num_modes, self.t, self.accept = o, A, 0, accept
        self.kws = []

    def _obs(self):
        return torch.full((self.num_envs, self.obs_dim ** 2), float(self.t), dtype=torch.float16)

    def reset(self):
        self.t = 0
        return self._obs(), {}

    def step(self, a, out=None):
        self.t += 1
        obs, rew, done = self._obs(), -a.abs().mean(dim=1), torch.full((self.num_envs,), self.t == self.max_steps)
        if out is not None:
            out[0].copy_(obs)
            out[1].copy_(rew)
            out[2].copy_(done)
        return obs, rew, done, None, {}

    def _kw(self, kw):
        if kw and not self.accept:
            raise TypeError(f"unexpected keywords {sorted(kw)}")
        self.kws.append(dict(kw))

    def reset_with_policy(self, policy, cov_var=0.5, policy_out=None, **kw):
        self._kw(kw)
        obs, info = self.reset()
        return (obs, info), policy.query(obs, policy_out, {})

    def step_with_policy(self, policy, cov_var=0.5, out=None, policy_out=None, action=None, **kw):
        self._kw(kw)
        ret = self.step(torch.zeros(self.num_envs, self.num_modes), out=out)
        if self.t == self.max_steps:
            return ret, None
        return ret, policy.query(ret[0], policy_out, {})


@pytest.mark.parametrize("fused", [False, True])
def test_keywords_reach_env_and_query_only_when_set(fused):
    B, o, A, T = 3, 2, 4, 3
    actor = make_actor(o * o, A, 8)
    # defaults: stand-ins that accept no new keyword run as before
    env, pol = RecEnv(B, o, A, T, accept=False), RecPolicy(accept=False)
    rollout(env, actor, episodes=2, actor_impl="hip", dev_actor=pol, fused_policy=fused)
    assert pol.calls == 2 * T and env.kws in ([], [{}] * 2 * (T + 1))
    for kw in ({"ou_noise": _cpu_ou(B, A)}, {"action_mode": "mean"}, {"ou_noise": _cpu_ou(B, A), "action_mode": "mean"}):
        env, pol = RecEnv(B, o, A, T, accept=True), RecPolicy(accept=True)
        rollout(env, actor, episodes=2, actor_impl="hip", dev_actor=pol, fused_policy=fused, **kw)
        seen = env.kws if fused else pol.kws
        assert len(seen) == (2 * (T + 1) if fused else 2 * T)
        for s in seen:
            assert set(s) == set(kw)
            assert all(s[k] is kw[k] for k in kw)
        if fused:
            assert pol.kws == [{}] * pol.calls   # (the env makes the query)
        else:
            assert env.kws == []
    # sample mode with no OU stays on the plain path even when the stand-ins would accept more
    env, pol = RecEnv(B, o, A, T, accept=True), RecPolicy(accept=True)
    rollout(env, actor, episodes=1, actor_impl="hip", dev_actor=pol, fused_policy=fused, action_mode="sample")
    assert all(k == {} for k in env.kws + pol.kws)


def test_torch_ou_is_still_added_outside_the_query():
    B, o, A, T = 2, 2, 3, 2
    ou = OrnsteinUhlenbeckNoise(B, A, 0.0, 0.0, 0.0)   # theta = sigma = 0: the state stays where it is put
    ou.state.fill_(1.0)
    env, pol = RecEnv(B, o, A, T, accept=False), RecPolicy(accept=False)
    out = rollout(env, make_actor(o * o, A, 8), episodes=1, actor_impl="hip", dev_actor=pol, ou_noise=ou)
    assert pol.kws == [{}] * T
    mean0 = torch.arange(A, dtype=torch.float32)   # obs 0 at the first step
    assert torch.equal(out["act"][0], (mean0 + 1.0).expand(B, A))


def test_rollout_refusals():
    B, o, A, T = 2, 2, 4, 3
    env = RecEnv(B, o, A, T, accept=True)
    actor = make_actor(o * o, A, 8)
    with pytest.raises(ValueError, match="actor_impl='hip'"):   # a DeviceOUNoise needs the HIP query
        rollout(env, actor, actor_impl="torch", ou_noise=_cpu_ou(B, A))
    with pytest.raises(ValueError, match="actor_impl='hip'"):   # "auto" resolves to the torch forward for a CPU module
        rollout(env, actor, ou_noise=_cpu_ou(B, A))
    with pytest.raises(ValueError, match="action_mode"):
        rollout(env, actor, actor_impl="hip", dev_actor=RecPolicy(True), action_mode="greedy")
    env.SH_operation = True
    with pytest.raises(ValueError, match="shack"):
        rollout(env, None, policy="shack", ou_noise=_cpu_ou(B, A))
    with pytest.raises(ValueError, match="shack"):
        rollout(env, None, policy="shack", action_mode="mean")
    with pytest.raises(ValueError, match="ou_noise"):   # the torch noise still cannot ride in the fused loop
        rollout(env, None, actor_impl="hip", dev_actor=RecPolicy(True), fused_policy=True, ou_noise=OrnsteinUhlenbeckNoise(B, A, 0.0, 0.3, 0.05))
    assert env.kws == []


def test_torch_mean_mode():
    """actor_impl='torch', action_mode='mean': the action is actor(obs) and log_prob the density of N(mean, cov_var I) at the mean."""
    B, o, A, T = 3, 2, 4, 2
    torch.manual_seed(0)
    actor = make_actor(o * o, A, 8)
    actor.eval()   # (no dropout here, so that the action can be recomputed)
    env = RecEnv(B, o, A, T, accept=False)
    out = rollout(env, actor, episodes=1, actor_impl="torch", action_mode="mean", cov_var=0.5)
    with torch.no_grad():
        for t in range(T):
            assert torch.equal(out["act"][t], actor(torch.full((B, o * o), float(t), dtype=torch.float16)))
    ref = torch.full((B,), -0.5 * A * math.log(2 * math.pi * 0.5), dtype=torch.float32)
    assert torch.equal(out["log_prob"], ref.expand(T, B))
