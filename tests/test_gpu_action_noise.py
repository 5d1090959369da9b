"""Action forms of the policy query on the device (aog_action_noise: mean mode, DDPG's Ornstein-Uhlenbeck term) through aog_actor_act_noise
and the fused tail (aog_reset_act_noise / aog_step_act_noise): exact composition with the plain query, the mean mode, fused against unfused
rollouts, a split batch against the whole, and the statistics of the OU process.  Fresh DeviceActors of the same module and seed give query
pairs at the same call index, as in test_gpu_step_act.py.

Bit-exact log_prob comparisons use act_dim 16: one output tile, so the log-probability's LDS atomics come from one instruction of one wave and
their order is fixed.  With more tiles that order is open (test_gpu_step_act.py compares log_prob to 1e-6 for that reason, and so do the
rollout comparisons here that use 64 units)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import smooth_screens

pytestmark = pytest.mark.gpu

SEED = 11


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _actor(S, A, H):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import make_actor

    torch.manual_seed(5)
    actor = make_actor(S, A, H, device="cuda:0")
    with torch.no_grad():   # a visible mean: the output layer's reference init (3e-3) would leave the mirror at the noise
        actor.out.weight.mul_(100.0)
    return actor


def _obs(B, S, seed):
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((B, S), generator=g).to(torch.float16).cuda()


def _start_state(ou, seed):
    """A nonzero OU state, float64."""
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(seed)
    ou.state.copy_((0.2 * torch.randn(ou.state.shape, generator=g, dtype=torch.float64)).cuda())


def _logp_const(A, cov_var):
    """The host's float32 constant 0.5 A log(2 pi cov_var) (actor_args: float arithmetic, libm's logf)."""
    logf = C.CDLL("libm.so.6").logf
    logf.restype, logf.argtypes = C.c_float, [C.c_float]
    f = np.float32
    return f(f(0.5) * f(A)) * f(logf(float(f(2.0) * f(np.pi) * f(cov_var))))


def _check_composition(torch, plain, noisy, s_before, s_after, ou):
    (a0, l0, m0), (a1, l1, m1) = plain, noisy
    assert torch.equal(a1, (a0.double() + s_after).float()), "action_ou != float32(float64(action_plain) + state_after)"
    assert torch.equal(m1, m0) and torch.equal(l1, l0)
    if ou.sigma == 0.0:
        s = s_before.cpu().numpy()
        np.testing.assert_array_equal(s_after.cpu().numpy(), s + ou.theta * (ou.mu - s))
    else:
        assert not torch.equal(s_after, s_before)


@pytest.mark.parametrize("sigma", [0.05, 0.0])
def test_composition_actor_act(sigma):
    """aog_actor_act_noise against aog_actor_act at the same call index (B = 70: a ragged last workgroup)."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise

    B, S, A, H = 70, 4, 16, 150
    actor = _actor(S, A, H)
    obs = _obs(B, S, 1)
    ou = DeviceOUNoise(B, A, mu=0.1, theta=0.3, sigma=sigma, device="cuda:0")
    _start_state(ou, 2)
    plain, noisy = DeviceActor(actor, seed=SEED), DeviceActor(actor, seed=SEED)
    for _ in range(3):
        s_before = ou.state.clone()
        r0 = [t.clone() for t in plain(obs)]
        r1 = [t.clone() for t in noisy(obs, ou_noise=ou)]
        torch.cuda.synchronize()
        _check_composition(torch, r0, r1, s_before, ou.state.clone(), ou)
    assert plain.calls == noisy.calls == 3


def _tail_env(B, A, T, seed):
    from adaptive_optics_gym_amd import BatchedAOEnv

    return BatchedAOEnv(B, "cuda:0", act_dim=A, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=T, screens=smooth_screens(B, 64, seed),
                        verbose=False)


@pytest.mark.parametrize("sigma", [0.05, 0.0])
def test_composition_fused_tail(sigma):
    """aog_reset_act_noise against aog_reset_act on identically built quasi-static envs: every reset observes the same screens with a flat
    mirror, so the query pairs see the same observation at the same call index (T = 1: the step queries nothing)."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise

    B, A, T = 70, 16, 1
    actor = _actor(4, A, 150)
    env0, env1 = _tail_env(B, A, T, 3), _tail_env(B, A, T, 3)
    ou = DeviceOUNoise(B, A, mu=-0.05, theta=0.3, sigma=sigma, device="cuda:0")
    _start_state(ou, 4)
    plain, noisy = DeviceActor(actor, seed=SEED), DeviceActor(actor, seed=SEED)
    for _ in range(3):
        s_before = ou.state.clone()
        (o0, _), r0 = env0.reset_with_policy(plain)
        (o1, _), r1 = env1.reset_with_policy(noisy, ou_noise=ou)
        r0, r1 = [t.clone() for t in r0], [t.clone() for t in r1]
        torch.cuda.synchronize()
        assert torch.equal(o0, o1)
        _check_composition(torch, r0, r1, s_before, ou.state.clone(), ou)
        s_mid = ou.state.clone()
        assert env0.step_with_policy(plain)[1] is None and env1.step_with_policy(noisy, ou_noise=ou)[1] is None
        torch.cuda.synchronize()
        assert torch.equal(ou.state, s_mid)   # the episode's last step queries nothing: the state stays
    assert plain.calls == noisy.calls == 3
    for env in (env0, env1):
        assert env.device_status() == 0
        env.close()


def test_mean_mode_actor_act():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor

    B, S, A, H, cov = 70, 4, 16, 150, 0.5
    actor = _actor(S, A, H)
    obs = _obs(B, S, 6)
    twin, mean_q = DeviceActor(actor, seed=SEED), DeviceActor(actor, seed=SEED)
    const = _logp_const(A, cov)
    for _ in range(3):
        a0, l0, m0 = [t.clone() for t in twin(obs, cov)]
        a1, l1, m1 = [t.clone() for t in mean_q(obs, cov, action_mode="mean")]
        torch.cuda.synchronize()
        assert torch.equal(a1, m0) and torch.equal(m1, m0), "mean mode: the action is the sample-mode twin's mean (same dropout)"
        assert not torch.equal(a0, m0)
        assert bool((l1 == torch.tensor(-const, device="cuda:0")).all()), (float(l1[0]), -float(const))


def test_mean_mode_fused_tail():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor

    B, A, T, cov = 70, 16, 1, 0.5
    actor = _actor(4, A, 150)
    env0, env1 = _tail_env(B, A, T, 7), _tail_env(B, A, T, 7)
    twin, mean_q = DeviceActor(actor, seed=SEED), DeviceActor(actor, seed=SEED)
    const = _logp_const(A, cov)
    for _ in range(2):
        _, (a0, l0, m0) = env0.reset_with_policy(twin, cov)
        _, (a1, l1, m1) = env1.reset_with_policy(mean_q, cov, action_mode="mean")
        torch.cuda.synchronize()
        assert torch.equal(a1, m0) and torch.equal(m1, m0)
        assert bool((l1 == torch.tensor(-const, device="cuda:0")).all())
        env0.step_with_policy(twin)
        env1.step_with_policy(mean_q, action_mode="mean")
    for env in (env0, env1):
        env.close()


# ---- fused against unfused rollouts ----------------------------------------------------------------------------------------------------

def _run(make_env, actor, fused, lookahead=False, episodes=2, ou=True, action_mode="sample"):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise, rollout

    envs = make_env()
    outs, tail, calls = [], [], []
    for env in envs:
        da = DeviceActor(actor, seed=SEED, env_id_base=env.global_env_offset)
        kw = {}
        if ou:
            kw["ou_noise"] = noise = DeviceOUNoise(env.num_envs, env.num_modes, 0.0, 0.3, 0.05, device="cuda:0")
        outs.append(rollout(env, actor, episodes=episodes, actor_impl="hip", dev_actor=da, lookahead=lookahead, fused_policy=fused,
                            action_mode=action_mode, **kw))
        if ou:
            tail.append(noise.state.clone())
        tail.append(env.get_actuators())
        if env.atm_type == "dynamic":
            tail.append(env.get_screens())
        assert env.device_status() == 0
        calls.append(da.calls)
    torch.cuda.synchronize()
    for env in envs:
        env.close()
    keys = ("obs", "next_obs", "act", "rew", "done", "log_prob")
    out = {k: torch.cat([o[k] for o in outs], dim=1) for k in keys}
    out["ep_returns"] = torch.cat([o["ep_returns"] for o in outs], dim=1)
    return out, tail, calls


def _check(ref, got, exact_log_prob=False):
    torch = _torch()
    (r, r_tail, r_calls), (g, g_tail, g_calls) = ref, got
    for k in ("obs", "next_obs", "act", "rew", "done", "ep_returns"):
        assert torch.equal(r[k], g[k]), f"{k}: fused differs from the unfused loop"
    if exact_log_prob:
        assert torch.equal(g["log_prob"], r["log_prob"])
    else:
        torch.testing.assert_close(g["log_prob"], r["log_prob"], rtol=1e-6, atol=0)
    assert len(r_tail) == len(g_tail)
    for a, b in zip(r_tail, g_tail):   # OU state, actuators, screens
        assert torch.equal(a, b)
    assert all(c == r_calls[0] for c in r_calls + g_calls)
    assert float(r["act"].abs().max()) > 0 and bool(torch.isfinite(r["rew"]).all())


def _compare(kw, B, S, A, H, lookahead=False, check_env=None, **run_kw):
    from adaptive_optics_gym_amd import BatchedAOEnv

    actor = _actor(S, A, H)

    def make():
        env = BatchedAOEnv(B, "cuda:0", **kw)
        if check_env is not None:
            check_env(env)
        return [env]

    _check(_run(make, actor, False, lookahead, **run_kw), _run(make, actor, True, lookahead, **run_kw))


@pytest.mark.parametrize("lookahead", [False, True])
def test_fused_ou_dynamic_int8_extrusion(lookahead):
    kw = dict(atm_type="dynamic", atm_vel=20.0, act_dim=16, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=5, seed=4,
              screen_oversampling=4, verbose=False)

    def check(env):
        assert env.extrusion_kmax >= 1   # the int8 composite extrusion

    _compare(kw, 40, 4, 16, 150, lookahead=lookahead, check_env=check)


def test_fused_ou_o5_ssim():
    kw = dict(atm_type="semi_dynamic", act_dim=16, obs_dim=5, rew_type="smf_ssim", rew_threshold=0.05, num_pupil_pixels=64,
              timesteps_per_episode=4, seed=6, screen_oversampling=4, verbose=False)
    _compare(kw, 33, 25, 16, 150)


def test_fused_ou_separable_o8():
    kw = dict(act_dim=64, obs_dim=8, num_pupil_pixels=64, timesteps_per_episode=4, screens=smooth_screens(20, 64, 2), verbose=False)

    def check(env):
        assert env.obs_route == "separable"

    _compare(kw, 20, 64, 64, 150, check_env=check)


def test_fused_ou_ragged_b1000():
    kw = dict(act_dim=64, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=3, seed=3, screen_oversampling=4, verbose=False)
    _compare(kw, 1000, 4, 64, 150)


def test_fused_mean_mode():
    kw = dict(act_dim=16, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=4, screens=smooth_screens(36, 64, 9), verbose=False)
    _compare(kw, 36, 4, 16, 150, ou=False, action_mode="mean")


def test_split_batch_matches_one_handle():
    """Two handles of B / 2 (env_id_base 0 and B / 2), each with its own DeviceOUNoise, through the fused path = one handle of B through the
    unfused loop, OU states included."""
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N = 64, 64
    scr = smooth_screens(B, N, 7)
    kw = dict(act_dim=16, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=4, verbose=False)
    actor = _actor(4, 16, 150)
    whole = _run(lambda: [BatchedAOEnv(B, "cuda:0", screens=scr, **kw)], actor, False)
    split = _run(lambda: [BatchedAOEnv(B // 2, "cuda:0", screens=scr[h * B // 2:(h + 1) * B // 2], global_env_offset=h * B // 2, total_envs=B, **kw)
                          for h in range(2)], actor, True)
    torch = _torch()
    # whole tail: [state, actuators]; split: [state_0, actuators_0, state_1, actuators_1]
    s_split = torch.cat([split[1][0], split[1][2]], dim=0)
    a_split = torch.cat([split[1][1], split[1][3]], dim=0)
    _check((whole[0], list(whole[1]), whole[2][:1]), (split[0], [s_split, a_split], split[2]), exact_log_prob=True)


# ---- statistics of the OU process ------------------------------------------------------------------------------------------------------

def test_ou_statistics():
    """B = 1024, A = 64, theta 0.3, sigma 0.05, 40 queries from s = mu.  n recovered from the state recursion, eps from the plain twin's action.
    The bounds are 5-sigma conditions (numpy's generator with the reference recursion uses at most 0.68 of each at these sizes)."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise

    B, S, A, H, K = 1024, 4, 64, 150, 40
    mu, theta, sigma, cov = 0.0, 0.3, 0.05, 0.5
    N = B * A
    actor = _actor(S, A, H)
    obs = _obs(B, S, 12)
    ou = DeviceOUNoise(B, A, mu, theta, sigma, device="cuda:0")
    plain, noisy = DeviceActor(actor, seed=SEED), DeviceActor(actor, seed=SEED)
    std = math.sqrt(cov)
    prev = None
    worst = {}

    def use(name, value, bound):
        worst[name] = max(worst.get(name, 0.0), abs(value) / bound)
        assert abs(value) <= bound, (name, k, value, bound)

    for k in range(1, K + 1):
        s_old = ou.state.cpu().numpy().copy()
        a0, _, m0 = plain(obs, cov)
        noisy(obs, cov, ou_noise=ou)
        s = ou.state.cpu().numpy()
        n = ((s - s_old - theta * (mu - s_old)) / sigma).ravel()
        eps = ((a0.double() - m0.double()) / std).cpu().numpy().ravel()
        use("mean", n.mean(), 5 / math.sqrt(N))
        use("var", n.var() - 1, 5 * math.sqrt(2 / N))
        use("corr", np.corrcoef(n, eps)[0, 1], 5 / math.sqrt(N))
        v = sigma ** 2 * (1 - (1 - theta) ** (2 * k)) / (1 - (1 - theta) ** 2)
        use("stat_var", ((s - mu) ** 2).mean() / v - 1, 5 * math.sqrt(2 / N))
        if k > 20:
            use("lag1", np.corrcoef(prev.ravel(), s.ravel())[0, 1] - (1 - theta), 5 * (1 - (1 - theta) ** 2) / math.sqrt(N))
        prev = s.copy()
    print({name: round(w, 3) for name, w in worst.items()}, "(largest fraction of each bound used over the 40 queries)")
