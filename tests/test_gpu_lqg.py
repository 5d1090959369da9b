"""The LQG controller on the device (include/aogym_lqg.h, csrc/k_lqg.h) against its host replay (tests/lqg_reference.py), bit for bit, and
through ``LQGController`` and ``rollout(policy="lqg")``.

Shapes: B = 5, A = 70 (rows that are no multiple of a wave, a mode index that crosses lane 64, three envs per workgroup of the update and
two workgroups) and B = 1, A = 1; S in {1, 2, 4}, delay in {1, 4}, 64 Riccati iterations; random stable models with poles inside radius
0.98, q and r in [1e-3, 1]."""
import types

import numpy as np
import pytest

import lqg_reference as ref

pytestmark = pytest.mark.gpu

STEPS, ITER = 48, 64


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0").contiguous()


def _case(B, A, S, seed=0):
    """A random stable model and STEPS rows of measurements, on the host."""
    rng = np.random.default_rng(1000 * S + 10 * A + B + seed)
    a, q, r = ref.random_stable_model(rng, B, S, A)
    return a, q, r, rng.standard_normal((STEPS, B, A))


def _filter(torch, B, A, S, model=None):
    from adaptive_optics_gym_amd.lqg import DeviceLQG

    f = DeviceLQG(B, A, S, device="cuda:0")
    if model is not None:
        f.set_model(*(_dev(torch, v) for v in model))
    return f


def _same_records(torch, f, rep, names=("a", "q", "r", "K", "c", "convergence", "solved", "xhat", "command")):
    got = f.unpack()
    want = {"a": rep.a, "q": rep.q, "r": rep.r, "K": rep.K, "c": rep.c, "convergence": rep.conv, "solved": rep.solved, "xhat": rep.xhat,
            "command": rep.command}
    for name in names:
        assert torch.equal(got[name].cpu(), torch.from_numpy(want[name])), name


# ---- 1. bit-exact replay -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,S,delay", [(5, 70, 1, 1), (5, 70, 2, 4), (5, 70, 4, 1), (5, 70, 4, 4), (1, 1, 2, 1), (1, 1, 4, 4)])
def test_solve_and_update_replay_bit_for_bit(B, A, S, delay):
    torch = _torch()
    a, q, r, ys = _case(B, A, S)
    rep = ref.LQGReference(B, A, S)
    rep.set_model(a, q, r)
    f = _filter(torch, B, A, S, (a, q, r))
    _same_records(torch, f, rep)
    conv = f.solve(delay, ITER)
    want = rep.solve(delay, ITER)
    assert np.isfinite(want).all() and np.abs(rep.K).max() > 0
    assert torch.equal(conv.cpu(), torch.from_numpy(want))
    _same_records(torch, f, rep)
    for t in range(STEPS):
        out = f.update(_dev(torch, ys[t]))
        assert torch.equal(out.cpu(), torch.from_numpy(rep.update(ys[t]))), t
        _same_records(torch, f, rep, ("xhat", "command"))
    assert float(out.abs().max()) > 0
    _same_records(torch, f, rep)
    f.close()


def test_a_row_with_a_nan_freezes_its_env_and_no_other():
    torch = _torch()
    B, A, S = 5, 70, 2
    a, q, r, ys = _case(B, A, S, seed=1)
    ys[10, 2, 69] = np.nan
    ys[11, 0, 0] = np.inf
    rep = ref.LQGReference(B, A, S)
    rep.set_model(a, q, r)
    rep.solve(2, ITER)
    f = _filter(torch, B, A, S, (a, q, r))
    f.solve(2, ITER)
    for t in range(14):
        before = f.unpack()
        out = f.update(_dev(torch, ys[t]))
        assert torch.equal(out.cpu(), torch.from_numpy(rep.update(ys[t]))), t
        _same_records(torch, f, rep, ("xhat", "command"))
        frozen = {10: 2, 11: 0}.get(t)
        if frozen is not None:
            after = f.unpack()
            assert torch.equal(after["xhat"][frozen], before["xhat"][frozen]) and torch.equal(out[frozen], before["command"][frozen])
            others = [b for b in range(B) if b != frozen]
            assert not torch.equal(after["xhat"][others], before["xhat"][others])
    assert bool(torch.isfinite(f.get_state().view(torch.float64)).all())
    f.close()


# ---- 2. the state machine ------------------------------------------------------------------------------------------------------------------------
def test_masks_leave_unselected_envs_untouched_and_update_needs_gains():
    torch = _torch()
    from adaptive_optics_gym_amd._lib import AogError

    B, A, S = 5, 70, 2
    a, q, r, ys = _case(B, A, S, seed=2)
    a2, q2, r2, _ = _case(B, A, S, seed=3)
    mask = np.array([True, False, True, True, False])
    rep = ref.LQGReference(B, A, S)
    f = _filter(torch, B, A, S)
    y0 = _dev(torch, ys[0])
    with pytest.raises(AogError, match="aog_lqg_update: no gains"):
        f.update(y0)
    rep.set_model(a, q, r), f.set_model(_dev(torch, a), _dev(torch, q), _dev(torch, r))
    with pytest.raises(AogError, match="aog_lqg_update: no gains"):
        f.update(y0)
    rep.solve(1, ITER), f.solve(1, ITER)
    for t in range(3):
        assert torch.equal(f.update(_dev(torch, ys[t])).cpu(), torch.from_numpy(rep.update(ys[t])))
    # a second model for the masked envs: the others keep model, gains and filter state; update is refused until solve has run again
    rep.set_model(a2, q2, r2, mask), f.set_model(_dev(torch, a2), _dev(torch, q2), _dev(torch, r2), mask=torch.as_tensor(mask))
    _same_records(torch, f, rep)
    tm = torch.from_numpy(mask)
    K = f.unpack()["K"].cpu()
    assert not K[tm].any() and K[~tm].any()
    with pytest.raises(AogError, match="aog_lqg_update: no gains"):
        f.update(y0)
    conv = f.solve(3, ITER, mask=mask.tolist())
    want = rep.solve(3, ITER, mask)
    assert torch.equal(conv.cpu()[tm], torch.from_numpy(want)[tm]) and not conv.cpu()[~tm].any()   # (a fresh tensor: rows left out hold zeros)
    _same_records(torch, f, rep)
    for t in range(3, 8):
        m = mask if t % 2 else ~mask
        assert torch.equal(f.update(_dev(torch, ys[t]), mask=torch.as_tensor(m, device="cuda:0")).cpu(), torch.from_numpy(rep.update(ys[t], m))), t
        _same_records(torch, f, rep)
    rep.reset(~mask), f.reset(mask=(~mask).tolist())
    _same_records(torch, f, rep)
    got = {k: v.cpu() for k, v in f.unpack().items()}
    assert not got["xhat"][~tm].any() and got["xhat"][tm].any() and got["K"].any(dim=1).all()
    f.close()


# ---- 3. split, resume, streams -----------------------------------------------------------------------------------------------------------------
def test_a_split_batch_reproduces_the_whole():
    torch = _torch()
    B, A, S = 5, 70, 4
    a, q, r, ys = _case(B, A, S, seed=4)
    whole = _filter(torch, B, A, S, (a, q, r))
    parts = [(_filter(torch, hi - lo, A, S, (a[lo:hi], q[lo:hi], r[lo:hi])), lo, hi) for lo, hi in ((0, 2), (2, 5))]
    conv = whole.solve(4, ITER)
    assert torch.equal(conv, torch.cat([p.solve(4, ITER) for p, _, _ in parts]))
    for t in range(STEPS):
        out = whole.update(_dev(torch, ys[t]))
        assert torch.equal(out, torch.cat([p.update(_dev(torch, ys[t, lo:hi])) for p, lo, hi in parts])), t
    blob = whole.get_state().view(torch.float64).reshape(B, -1)
    assert torch.equal(blob, torch.cat([p.get_state().view(torch.float64).reshape(hi - lo, -1) for p, lo, hi in parts]))
    for f in [whole] + [p for p, _, _ in parts]:
        f.close()


def _stub_env(B, A):
    return types.SimpleNamespace(num_envs=B, num_modes=A, device="cuda:0", pyramid=None, global_env_offset=0)


def test_a_state_dict_resumes_without_solving_again():
    torch = _torch()
    from adaptive_optics_gym_amd import LQGController

    B, A = 5, 70
    a, q, r, ys = _case(B, A, 2, seed=5)
    line = dict(frequency=0.12, damping=0.01, ratio=0.25)
    first = LQGController(_stub_env(B, A), delay=2, vibrations=[line])
    assert float(first.convergence.max()) <= 1e-9
    first.set_model(_dev(torch, a), _dev(torch, q), _dev(torch, r))   # the caller's own model: a fresh controller's gains are not these
    first.solve()
    for t in range(20):
        first.update(_dev(torch, ys[t]))
    state = first.state_dict()
    second = LQGController(_stub_env(B, A), delay=2, vibrations=[line])
    assert not torch.equal(second.filter.unpack()["K"], first.filter.unpack()["K"])
    second.load_state_dict(state)
    solves = []
    second.filter.solve = lambda *args, **kw: solves.append(args)
    for t in range(20, STEPS):
        assert torch.equal(first.update(_dev(torch, ys[t])), second.update(_dev(torch, ys[t]))), t
    assert not solves and torch.equal(first.filter.get_state(), second.filter.get_state())
    assert torch.equal(first.telemetry.get_state(), second.telemetry.get_state()) and torch.equal(first.command, second.command)
    assert torch.equal(second.a, first.a) and first.telemetry.unpack()["count"].tolist() == [STEPS] * B
    # a blob that holds no gains is refused by update after it is loaded, as before solve
    from adaptive_optics_gym_amd._lib import AogError

    bare = _filter(torch, B, A, 2, (a, q, r))
    second.filter.set_state(bare.get_state())
    with pytest.raises(AogError, match="aog_lqg_update: no gains"):
        second.update(_dev(torch, ys[0]))
    with pytest.raises(ValueError, match="delay = 2"):
        LQGController(_stub_env(B, A), delay=1, vibrations=[line]).load_state_dict(state)
    bare.close(), first.close(), second.close()


def test_a_side_stream_run_equals_the_default_stream_run():
    torch = _torch()
    B, A, S = 5, 70, 2
    a, q, r, ys = _case(B, A, S, seed=6)
    mask = torch.tensor([True, True, False, True, True], device="cuda:0")

    def run():
        f = _filter(torch, B, A, S, (a, q, r))
        outs = [f.solve(2, ITER)]
        for t in range(12):
            outs.append(f.update(_dev(torch, ys[t]), mask=mask if t == 5 else None))
        f.reset(mask=mask)
        outs.append(f.update(_dev(torch, ys[12])))
        blob = f.get_state()
        g = _filter(torch, B, A, S)
        g.set_state(blob)
        outs += [g.update(_dev(torch, ys[13])), g.get_state()]
        torch.cuda.current_stream().synchronize()
        f.close(), g.close()
        return outs

    want = run()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)


# ---- 4. the loop runs ----------------------------------------------------------------------------------------------------------------------------
N, LB, LA, LT = 32, 4, 9, 24
KEYS = ("obs", "act", "log_prob", "rew", "next_obs", "done")


def _loop_env(servo):
    from adaptive_optics_gym_amd import LayeredAOEnv
    from adaptive_optics_gym_amd.params import OpticalParams

    dt = float(OpticalParams(num_pupil_pixels=N).delta_t)
    kw = dict(atm_layers=[{"fraction": 0.6, "speed": 10.0}, {"fraction": 0.4, "speed": 15.0}], atm_fried=0.15, seed=11, act_type="zernike", act_dim=LA,
              obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=LT, num_pupil_pixels=N, verbose=False, SH_operation=True,
              disturbance=dict(shapes=["tip"], vibrations=[dict(term=0, frequency=0.12 / dt, damping=0.01, rms=5e-8)]))
    if servo is not None:
        kw["servo"] = servo
    return LayeredAOEnv(LB, "cuda:0", **kw)


@pytest.mark.parametrize("servo,delay", [(None, 1), (dict(latency=1), 2)], ids=["no_servo", "latency_1"])
def test_rollout_with_the_lqg_policy_equals_a_hand_written_loop(servo, delay):
    torch = _torch()
    from adaptive_optics_gym_amd import LQGController
    from adaptive_optics_gym_amd.rollout import rollout

    envs = [_loop_env(servo) for _ in range(2)]
    line = dict(frequency=0.12, damping=0.01, ratio=1.0)
    ctrls = [LQGController(e, measurement="truth", delay=delay, vibrations=[line]) for e in envs]
    got = rollout(envs[0], None, episodes=1, policy="lqg", controller=ctrls[0])
    rows = {k: [] for k in KEYS}
    with torch.no_grad():
        obs, _ = envs[1].reset()
        for t in range(LT):
            action = ctrls[1].action().float().clone()
            ret = envs[1].step(action)
            for k, v in zip(KEYS, (obs, action, torch.ones(LB, device="cuda"), ret[1], ret[0], ret[2])):
                rows[k].append(v.clone())
            obs = ret[0]
    for k in KEYS:
        want = torch.stack(rows[k])
        assert got[k].shape == want.shape and got[k].dtype == want.dtype and torch.equal(got[k], want), k
        assert bool(torch.isfinite(got[k].float()).all()), k
    assert tuple(got["act"].shape) == (LT, LB, LA) and float(got["act"].abs().max()) > 0
    assert torch.equal(ctrls[0].filter.get_state(), ctrls[1].filter.get_state())
    assert ctrls[0].telemetry.unpack()["count"].tolist() == [LT] * LB
    for c, e in zip(ctrls, envs):
        c.close()
        e.close()
