"""rollout()'s policy table against loops written here from public calls only (env.reset, the action source, env.step), bit for bit, on twin
envs built from the same seed: the policies no other test holds to such a loop.  Those that are held to one elsewhere:
"ideal" in test_gpu_wavefront_truth.py::test_rollout_with_the_ideal_policy, "pyramid" and "predictive" in
test_gpu_telemetry.py::test_the_other_policies_keep_their_bits.

Smallest shapes: 3 envs, obs_dim 2, one mode (the library takes act_dim >= 1), T = 3, 2 episodes; the controllers start from a state in which
one env was reset under a mask."""
import pytest

pytestmark = pytest.mark.gpu

B, A, T, E = 3, 1, 3, 2
KW = dict(atm_type="dynamic", atm_vel=20.0, act_dim=A, obs_dim=2, num_pupil_pixels=32, screen_oversampling=4, timesteps_per_episode=T, seed=17,
          verbose=False)
MASK = [False, True, False]
KEYS = ("obs", "act", "log_prob", "rew", "next_obs", "done")


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _twins(**kw):
    _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    return [BatchedAOEnv(B, "cuda:0", **dict(KW, **kw)) for _ in range(2)]


def _loop(env, first_action, next_action):
    """The reference: E episodes of reset, T x (action, step).  first_action(obs) -> (action, log_prob) of an episode's first step,
    next_action(obs, step tuple) -> those of every later one (log_prob None: the constant 1)."""
    torch = _torch()
    rows = {k: [] for k in KEYS}
    returns = []
    with torch.no_grad():
        for _ in range(E):
            obs, _ = env.reset()
            ret = None
            for t in range(T):
                action, log_prob = first_action(obs) if t == 0 else next_action(obs, ret)
                action = action.float().clone()
                ret = env.step(action)
                for k, v in zip(KEYS, (obs, action, torch.ones(B, device="cuda") if log_prob is None else log_prob, ret[1], ret[0], ret[2])):
                    rows[k].append(v.clone())
                obs = ret[0]
            returns.append(torch.stack(rows["rew"][-T:]).sum(0))
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["ep_returns"] = torch.stack(returns)
    return out


def _same(got, want, log_prob_rtol=None):
    torch = _torch()
    assert tuple(got["act"].shape) == (T * E, B, A) and tuple(got["obs"].shape) == (T * E, B, 4)
    for k in KEYS + ("ep_returns",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if k == "log_prob" and log_prob_rtol is not None:
            torch.testing.assert_close(got[k], want[k], rtol=log_prob_rtol, atol=0)
        else:
            assert torch.equal(got[k], want[k]), k
    assert got["avg_ep_rew"] == float(want["ep_returns"].mean().item()) / T
    assert got["batch_lens"].tolist() == [T] * E + [0] * (T * E - E)
    assert bool(got["done"][T - 1::T].all()) and not bool(got["done"][:T - 1].any())
    assert float(got["act"].abs().max()) > 0


def _actor():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import make_actor

    torch.manual_seed(5)
    actor = make_actor(4, A, 32, device="cuda:0")
    with torch.no_grad():   # a visible mean: the output layer's reference init (3e-3) would leave the mirror at the noise
        actor.out.weight.mul_(100.0)
    return actor


def test_actor_torch_query():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import rollout, sample_action

    one, two = _twins()
    actor = _actor()
    gen = torch.Generator(device="cuda")
    torch.manual_seed(3)   # (the module's dropout draws from the global generator, the action's noise from gen)
    gen.manual_seed(4)
    got = rollout(one, actor, episodes=E, actor_impl="torch", generator=gen)
    torch.manual_seed(3)
    gen.manual_seed(4)
    act = lambda obs, ret=None: sample_action(actor(obs), 0.5, gen)
    _same(got, _loop(two, act, act))
    one.close()
    two.close()


@pytest.mark.parametrize("fused", [False, True])
def test_actor_hip_query(fused):
    """log_prob to 1e-6, as in test_gpu_step_act.py: aog_actor_act sums it with float atomics, in an unfixed order."""
    _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, rollout

    one, two = _twins()
    actor = _actor()
    got = rollout(one, actor, episodes=E, actor_impl="hip", dev_actor=DeviceActor(actor, seed=9), fused_policy=fused)
    da = DeviceActor(actor, seed=9)
    act = lambda obs, ret=None: da(obs)[:2]
    _same(got, _loop(two, act, act), log_prob_rtol=1e-6)
    assert da.calls == T * E
    one.close()
    two.close()


def test_shack():
    _torch()
    from adaptive_optics_gym_amd.rollout import rollout

    one, two = _twins(SH_operation=True)
    got = rollout(one, None, episodes=E, policy="shack")
    act = lambda obs, ret=None: (two.SH_step()[0], None)
    _same(got, _loop(two, act, act))
    one.close()
    two.close()


def test_modal():
    torch = _torch()
    from adaptive_optics_gym_amd import ModalIntegrator, ModalTelemetry
    from adaptive_optics_gym_amd.rollout import rollout

    envs = _twins(SH_operation=True)
    ctrls = [ModalIntegrator(e, measurement="truth", gain=0.4, telemetry=ModalTelemetry(B, A, length=64, device=e.device)) for e in envs]
    y0 = 1e-8 * torch.arange(1, B * A + 1, dtype=torch.float64, device="cuda").reshape(B, A)
    for c in ctrls:   # a command and a ring that differ from env to env: one update, then env 1 alone reset
        c.update(y0)
        c.reset(MASK)
    got = rollout(envs[0], None, episodes=E, policy="modal", controller=ctrls[0])
    act = lambda obs, ret=None: (ctrls[1].action(), None)
    _same(got, _loop(envs[1], act, act))
    assert torch.equal(ctrls[0].command, ctrls[1].command) and torch.equal(ctrls[0].telemetry.get_state(), ctrls[1].telemetry.get_state())
    assert ctrls[0].telemetry.unpack()["count"].tolist() == [T * E + 1, T * E, T * E + 1]
    for c, e in zip(ctrls, envs):
        c.close()
        e.close()


@pytest.mark.parametrize("fused", [False, True])
def test_spgd(fused):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import rollout
    from adaptive_optics_gym_amd.sensorless import SPGDController

    envs = _twins(SH_operation=True)
    ctrls = [SPGDController(e, gain=2e-6, amplitude=[2e-8, 3e-8, 4e-8], metric="strehl", seed=2024) for e in envs]
    metric = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float32, device="cuda")
    for c in ctrls:   # iteration counters that differ from env to env: env 1 alone has made two queries
        c.reset()
        c.update(metric, mask=MASK)
        c.update(metric, mask=MASK)
    got = rollout(envs[0], None, episodes=E, policy="spgd", controller=ctrls[0], fused_policy=fused)
    # (the controller is reset with the env; every later step queries it on the last step's metric)
    _same(got, _loop(envs[1], lambda obs: (ctrls[1].reset(), None), lambda obs, ret: (ctrls[1].update(ctrls[1].step_metric(ret)), None)))
    assert torch.equal(ctrls[0].get_state(), ctrls[1].get_state())
    k = ctrls[0].unpack()["k"].tolist()
    assert k[0] == k[2] != k[1]   # (env 1's own queries are still in its counter)
    for c, e in zip(ctrls, envs):
        c.close()
        e.close()
