"""The mirror servo on the device (aog_servo_apply: k_servo_apply, k_servo_reset) against the host restatement tests/servo_reference.py, bit
for bit, and through ``BatchedAOEnv(servo=...)`` / ``LayeredAOEnv(servo=...)``.  Shapes: B in {3, 67} (neither a multiple of a wave; 67 x 64 is
17 workgroups of 256 threads with the last three quarters empty, 3 x 5 one workgroup of 15 threads), A in {5, 64}."""
import numpy as np
import pytest

import servo_reference as ref
from checkpoint_harness import drive_with, resume_case
from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

N = 32
SHAPES = [(3, 5), (67, 64), (3, 64), (67, 5)]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class _Batch:
    """What a servo needs of an env: the batch, the action width, the global env ids and the device."""

    def __init__(self, torch, B, A, offset=0, total=None):
        self.num_envs, self.num_modes, self.global_env_offset, self.total_envs = B, A, offset, B + offset if total is None else total
        self.device = torch.device("cuda", 0)


def _params(B, A, max_latency=2):
    """Per-env latencies {0, 1, 1.5, max}, responses {1, 0.5, 0.1}, a finite stroke on every second env and two stuck actuators."""
    e = np.arange(B)
    latency = np.array([0.0, 1.0, 1.5, float(max_latency)])[e % 4]
    response = np.array([1.0, 0.5, 0.1])[e % 3]
    stroke = np.where(e % 2 == 1, 0.75, np.inf)
    stuck = np.zeros((B, A), dtype=bool)
    stuck[:, 1] = True
    stuck[e % 2 == 0, A - 1] = True
    value = np.where(stuck, np.float32(0.125), np.float32(0)).astype(np.float32) * np.float32(-1) ** np.arange(A, dtype=np.float32)
    return dict(latency=latency, response=response, stroke=stroke, stuck=(stuck, value), max_latency=max_latency)


def _pair(torch, B, A, offset=0, total=None, rows=slice(None), **kw):
    """A device servo over the envs ``rows`` of the parameters ``kw`` and its host replay."""
    from adaptive_optics_gym_amd import MirrorServo

    cut = {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if "stuck" in cut:
        cut["stuck"] = tuple(x[rows] for x in cut["stuck"])
    n = len(np.arange(B)[rows])
    dev = MirrorServo(_Batch(torch, n, A, offset, total), **cut)
    stuck, value = cut.get("stuck", (None, None))
    if any(isinstance(v, np.ndarray) and v.shape[0] != n for v in cut.values()):   # (values for total_envs: the device servo cuts them)
        return dev, None
    host = ref.Servo(n, A, dev.max_latency, cut.get("latency", 0.0), cut.get("response", 1.0), cut.get("stroke", np.inf), stuck, value)
    return dev, host


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(torch, got, want, what):
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want), err_msg=what)


def _acts(torch, B, A, t):
    a = actions_for(B, A, 40 + t)
    return a, torch.from_numpy(a).cuda()


# ---- 1. replay -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", SHAPES)
def test_replay_is_bit_identical(B, A):
    """12 calls on random float32 actions with a masked apply (call 5) and a masked reset (before call 8) in the middle."""
    torch = _torch()
    dev, host = _pair(torch, B, A, **_params(B, A))
    mask = np.arange(B) % 3 != 1
    try:
        assert dev._state_bytes() == host.blob().size == 8 * B * A + 8 + 4 * B * 4 * A
        moved = 0
        for t in range(12):
            a, a_dev = _acts(torch, B, A, t)
            if t == 8:
                dev.reset(torch.from_numpy(~mask).cuda())
                host.reset(~mask)
            if t == 5:
                out = torch.full((B, A), 7.0, device="cuda")
                got = dev.apply(a_dev, torch.from_numpy(mask).cuda(), out=out)
                want = host.apply(a, mask, out=np.full((B, A), np.float32(7)))
                assert got is out and bool((got[torch.from_numpy(~mask).cuda()] == 7).all())
            else:
                got, want = dev.apply(a_dev), host.apply(a)
            _same(torch, got, want, f"call {t}")
            moved += int(np.any(_bits(want) != _bits(a)))
            np.testing.assert_array_equal(dev.get_state().cpu().numpy(), host.blob(), err_msg=f"state after call {t}")
        assert moved == 12   # (the servo did something in every call)
    finally:
        dev.close()


@pytest.mark.parametrize("B,A", SHAPES[:2])
def test_the_identity_configuration_returns_its_input_bits(B, A):
    torch = _torch()
    for kw in (dict(), dict(max_latency=4), dict(latency=0.0, response=1.0, stroke=np.inf, stuck=(np.zeros(A, dtype=bool), np.zeros(A)))):
        dev, _ = _pair(torch, B, A, **kw)
        try:
            for t in range(3):
                a, a_dev = _acts(torch, B, A, t)
                a[0, 0] = -0.0
                a_dev = torch.from_numpy(a).cuda()
                _same(torch, dev.apply(a_dev), a, f"{kw}: call {t}")
            assert dev.apply(a_dev, out=a_dev) is a_dev   # (in place)
            _same(torch, a_dev, a, "in place")
        finally:
            dev.close()


# ---- 2. split batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,cut", [(3, 5, 2), (67, 64, 33)])
def test_parts_of_a_batch_reproduce_the_whole(B, A, cut):
    torch = _torch()
    p = _params(B, A)
    whole, _ = _pair(torch, B, A, **p)
    parts = [_pair(torch, B, A, 0, B, slice(0, cut), **p)[0], _pair(torch, B, A, cut, B, slice(cut, B), **p)[0]]
    # the same per-env values given for total_envs are cut at the global env id
    by_id = _pair(torch, B - cut, A, cut, B, **dict(p, stuck=tuple(x[cut:] for x in p["stuck"])))[0]
    mask = np.arange(B) % 3 != 1
    try:
        for t in range(7):
            _, a = _acts(torch, B, A, t)
            m = torch.from_numpy(mask).cuda() if t == 3 else None
            if t == 5:
                whole.reset(torch.from_numpy(~mask).cuda())
                for h, rows in ((parts[0], slice(0, cut)), (parts[1], slice(cut, B)), (by_id, slice(cut, B))):
                    h.reset(torch.from_numpy(~mask[rows]).cuda())
            want = whole.apply(a, m)
            got = [h.apply(a[rows].contiguous(), None if m is None else m[rows].contiguous())
                   for h, rows in ((parts[0], slice(0, cut)), (parts[1], slice(cut, B)), (by_id, slice(cut, B)))]
            assert torch.equal(torch.cat(got[:2]).view(torch.int32), want.view(torch.int32)), f"call {t}"
            assert torch.equal(got[2].view(torch.int32), want[cut:].view(torch.int32)), f"call {t}, per-env values by global id"
    finally:
        for h in [whole, by_id] + parts:
            h.close()


# ---- 3. checkpoint -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", SHAPES[:2])
def test_servo_checkpoint_resumes_bit_identically(B, A):
    torch = _torch()
    dev, _ = _pair(torch, B, A, **_params(B, A))
    other, _ = _pair(torch, B, A, **_params(B, A))
    try:
        for t in range(5):
            dev.apply(_acts(torch, B, A, t)[1])
        snap = dev.state_dict()
        first = [dev.apply(_acts(torch, B, A, t)[1]).clone() for t in range(5, 10)]
        end = dev.get_state()
        for h, what in ((dev, "the same servo after it has moved on"), (other, "a fresh servo")):
            h.load_state_dict(snap)
            again = [h.apply(_acts(torch, B, A, t)[1]) for t in range(5, 10)]
            for t, (x, y) in enumerate(zip(first, again)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: call {t} after the snapshot"
            assert torch.equal(h.get_state(), end), what
        wrong, _ = _pair(torch, B, A, max_latency=3)
        try:
            with pytest.raises(ValueError, match="another servo"):
                wrong.load_state_dict(snap)
            with pytest.raises(ValueError, match="blob"):
                wrong.set_state(snap["blob"])
        finally:
            wrong.close()
    finally:
        dev.close(), other.close()


def _env(B, A=5, T=6, act_type="zernike", **kw):
    from adaptive_optics_gym_amd import BatchedAOEnv

    base = dict(act_type=act_type, act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T, num_pupil_pixels=N, seed=17,
                screen_oversampling=4, verbose=False)
    base.update(kw)
    return BatchedAOEnv(B, "cuda:0", **base)


def test_env_checkpoint_carries_the_servo():
    B, T = 3, 4
    servo = dict(latency=[0.5, 1.0, 2.0], response=[0.5, 1.0, 0.25], stuck={2: 0.1})
    make = lambda: _env(B, T=T, atm_type="dynamic", atm_vel=20.0, servo=servo)
    drive = drive_with(T, after=lambda env: [env._last_action, env.servo.get_state()])
    assert resume_case(make, drive, 6, 5) > 0   # (the snapshot in mid-episode: the history holds commands)
    env, bare = make(), _env(B, T=T, atm_type="dynamic", atm_vel=20.0)
    try:
        env.reset(), bare.reset()
        with pytest.raises(ValueError, match="mirror servo"):
            bare.set_state(env.get_state())
        with pytest.raises(ValueError, match="mirror servo"):
            env.set_state(bare.get_state())
        assert "servo" not in bare.get_state()
    finally:
        env.close(), bare.close()


# ---- 4. through the env --------------------------------------------------------------------------------------------------------------------
def _outputs(ret):
    obs, reward, done, _, info = ret
    return [obs.clone(), reward.clone(), done.clone(), info["obs_raw"].clone(), info["power"].clone(), info["strehl"].clone()]


def _equal(torch, xs, ys, what):
    for j, (x, y) in enumerate(zip(xs, ys)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: output {j} differs"


@pytest.mark.parametrize("B,A,act_type", [(3, 5, "zernike"), (67, 64, "num_actuators")])
def test_env_with_the_identity_servo_returns_the_same_bits(B, A, act_type):
    torch = _torch()
    T = 4
    env, bare = _env(B, A, T, act_type, atm_type="semi_dynamic", servo=dict()), _env(B, A, T, act_type, atm_type="semi_dynamic")
    try:
        assert env.servo is not None and bare.servo is None and env.servo.max_latency == 0
        for t in range(T + 2):
            if t % T == 0:
                o0, o1 = env.reset()[0], bare.reset()[0]
                assert torch.equal(o0, o1)
            a = _acts(torch, B, A, t)[1]
            r0, r1 = env.step(a), bare.step(a)
            _equal(torch, _outputs(r0), _outputs(r1), f"step {t}")
            assert torch.equal(r0[4]["applied_action"].view(torch.int32), a.view(torch.int32)) and "applied_action" not in r1[4]
            assert env._last_action is r0[4]["applied_action"]
        assert bool(r0[2].any()) is False and env.timestep == T + 2
    finally:
        env.close(), bare.close()


@pytest.mark.parametrize("B,A,act_type", [(3, 5, "zernike"), (67, 64, "num_actuators")])
def test_env_with_two_frames_of_latency(B, A, act_type):
    """obs / power / strehl of step n are those of a servo-less twin stepped with action n - 2 (zeros before that); a masked reset in
    mid-episode restarts the history of those envs alone; info["applied_action"] is the replay's."""
    torch = _torch()
    T = 12
    scr = smooth_screens(B, N, 3)
    env, twin = _env(B, A, T, act_type, screens=scr, servo=dict(latency=2)), _env(B, A, T, act_type, screens=scr)
    host = ref.Servo(B, A, 2, latency=2.0)
    mask = np.arange(B) % 3 == 1
    try:
        env.reset(), twin.reset()
        acts = [_acts(torch, B, A, t) for t in range(9)]
        since = np.zeros(B, dtype=int)    # steps since each env's last reset
        for t in range(9):
            if t == 5:
                m = torch.from_numpy(mask).cuda()
                assert torch.equal(env.reset(m)[0], twin.reset(m)[0])
                host.reset(mask)
                since[mask] = 0
            old = np.stack([acts[t - 2][0][b] if since[b] >= 2 else np.zeros(A, dtype=np.float32) for b in range(B)])
            got, want = env.step(acts[t][1]), twin.step(torch.from_numpy(old).cuda())
            _equal(torch, _outputs(got), _outputs(want), f"step {t}")
            _same(torch, got[4]["applied_action"], host.apply(acts[t][0]), f"applied_action of step {t}")
            _same(torch, got[4]["applied_action"], old, f"applied_action of step {t} against the shifted commands")
            since += 1
        assert torch.equal(env.get_actuators(), twin.get_actuators())
        # set_actuators bypasses the servo and leaves it untouched
        blob = env.servo.get_state()
        env.set_actuators(torch.zeros((B, A), dtype=torch.float64, device="cuda"))
        assert torch.equal(env.servo.get_state(), blob) and not bool(env.get_actuators().any())
    finally:
        env.close(), twin.close()


def test_reset_leaves_the_servo_alone_without_a_flat_start():
    torch = _torch()
    B, A = 3, 5
    env = _env(B, A, flat_mirror_start_per_episode=False, servo=dict(latency=1, response=0.5))
    try:
        env.reset()
        for t in range(2):
            env.step(_acts(torch, B, A, t)[1])
        blob = env.servo.get_state()
        assert bool(blob.any())
        env.reset(), env.reset(torch.tensor([True, False, True]))
        assert torch.equal(env.servo.get_state(), blob)
    finally:
        env.close()


def test_layered_env_steps_its_sightline_with_the_applied_action():
    torch = _torch()
    from adaptive_optics_gym_amd import LayeredAOEnv

    B, A, T = 3, 5, 6
    kw = dict(atm_layers=[{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}], atm_fried=0.15, seed=11, layer_altitudes=[0.0, 1e4],
              sightlines={"up": (-4e-6, 1e-6)}, act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T,
              num_pupil_pixels=N, verbose=False)
    env, twin = LayeredAOEnv(B, "cuda:0", servo=dict(latency=1), **kw), LayeredAOEnv(B, "cuda:0", **kw)
    try:
        up = env.sightlines["up"]
        assert env.servo is not None and up.env.servo is None and all(lay.servo is None for lay in env.layers)
        env.reset(), twin.reset()
        zero = torch.zeros((B, A), device="cuda")
        acts = [_acts(torch, B, A, t)[1] for t in range(4)]
        for t in range(4):
            got, want = env.step(acts[t]), twin.step(acts[t - 1] if t else zero)
            _equal(torch, _outputs(got), _outputs(want), f"step {t}")
            # (bytes: step 0 applies the rest command 0, which the normalised action chain turns into 0 / 0 on both sides, as the reference does)
            mine, theirs = got[4]["sightlines"]["up"], want[4]["sightlines"]["up"]
            _equal(torch, [mine[k] for k in ("obs", "reward", "power", "strehl")], [theirs[k] for k in ("obs", "reward", "power", "strehl")],
                   f"step {t}: the sightline")
            assert t == 0 or bool(torch.isfinite(mine["obs"].float()).all() and torch.isfinite(mine["strehl"]).all())
            assert t == 0 or not torch.equal(mine["strehl"], got[4]["strehl"])   # (another line of sight: another wavefront)
            assert up.env._last_action is got[4]["applied_action"]
            _equal(torch, [up.env.get_actuators()], [env.get_actuators()], f"step {t}: the two fronts' actuators")
        with pytest.raises(RuntimeError, match="mirror servo"):
            env.step(acts[0], next_actions=acts[1])
        assert env.timestep == 4 and twin.timestep == 4 and env.layers[0].timestep == twin.layers[0].timestep   # (refused before the layers moved)
    finally:
        env.close(), twin.close()


# ---- 5. closed loop ------------------------------------------------------------------------------------------------------------------------
def _loop(torch, gain, servo, steps=60):
    """The residual integrator a <- a + g (ideal_action() - get_actuators()) on fixed screens: (rms at the start, rms at the end, fit_rms)."""
    B, A = 3, 20
    env = _env(B, A, 200, "num_actuators", screens=smooth_screens(B, N, 5, amp=1e-5, sigma_frac=0.15), SH_operation=True,
               **({} if servo is None else {"servo": servo}))
    try:
        env.reset()
        truth = env.wavefront_truth()
        start, fit = truth["rms"].clone(), truth["fit_rms"].clone()
        a = torch.zeros((B, A), dtype=torch.float64, device="cuda")
        for _ in range(steps):
            a = a + gain * (env.ideal_action() - env.get_actuators())
            env.step(a.to(torch.float32))
        return start.cpu().numpy(), env.wavefront_truth()["rms"].cpu().numpy(), fit.cpu().numpy()
    finally:
        env.close()


def test_closed_loop_falls_on_the_side_of_the_gain_limit_the_delay_sets():
    """With servo latency 1 the loop's delay is 2 frames and gain_limit(2) = 1: g = 0.8 converges to the fitting error, g = 1.2 diverges.
    Without the servo the delay is 1, gain_limit(1) = 2, and both converge."""
    torch = _torch()
    from adaptive_optics_gym_amd.telemetry import gain_limit

    assert gain_limit(1) == 2.0 and abs(gain_limit(2) - 1.0) < 1e-15
    for servo, gain, converges in ((dict(latency=1), 0.8, True), (dict(latency=1), 1.2, False), (None, 0.8, True), (None, 1.2, True)):
        start, end, fit = _loop(torch, gain, servo)
        print(f"servo {servo}, gain {gain}: rms {start.min():.3e} .. {start.max():.3e} m -> {end.min():.3e} .. {end.max():.3e} m; fit_rms "
              f"{fit.min():.3e} .. {fit.max():.3e} m; end / fit_rms - 1 = {np.max(end / fit - 1):.3e}")
        assert np.all(fit < 0.5 * start), "the screens leave the loop nothing to correct: the case checks nothing"
        if converges:
            assert np.all(np.abs(end / fit - 1.0) <= 0.01), f"servo {servo}, gain {gain}: the loop did not reach the fitting error"
        else:
            assert np.all(end > start), f"servo {servo}, gain {gain}: the loop should have left the stable side"


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_fused_and_pipelined_forms_are_refused():
    torch = _torch()
    from adaptive_optics_gym_amd import MirrorServo
    from adaptive_optics_gym_amd.rollout import rollout

    B, A = 3, 5
    env = _env(B, A, servo=dict(latency=1))
    try:
        env.reset()
        a = _acts(torch, B, A, 0)[1]
        first = _outputs(env.step(a))
        blob, clock = env.servo.get_state(), (env.timestep, env.observation_frames)
        calls = [lambda: env.step(a, next_actions=a), lambda: env.step(a, next_actions=None), lambda: env.step_with_policy(None),
                 lambda: env.reset_with_policy(None), lambda: env.step_with_spgd(None), lambda: env.reset_with_spgd(None)]
        for call in calls:
            with pytest.raises(RuntimeError, match="mirror servo"):
                call()
        with pytest.raises(ValueError, match="mirror servo"):
            rollout(env, None, policy="ideal", fused_policy=True)
        assert torch.equal(env.servo.get_state(), blob) and (env.timestep, env.observation_frames) == clock
        # the env is usable afterwards: the next step is that of a twin that was never refused anything
        twin = _env(B, A, servo=dict(latency=1))
        try:
            twin.reset()
            _equal(torch, _outputs(twin.step(a)), first, "the twin's first step")
            b = _acts(torch, B, A, 1)[1]
            _equal(torch, _outputs(env.step(b)), _outputs(twin.step(b)), "the step after the refusals")
        finally:
            twin.close()
    finally:
        env.close()
    # bad arguments raise before anything is created, and a ready servo must fit the env
    for bad in (dict(latency=5), dict(response=0.0), dict(gain=1.0), [1.0]):
        with pytest.raises(ValueError):
            _env(B, A, servo=bad)
    env = _env(B, A)
    try:
        other = MirrorServo(_Batch(torch, B, A + 1))
        with pytest.raises(ValueError, match="servo"):
            _env(B, A, servo=other)
        other.close()
        ready = MirrorServo(env, latency=1)
        owner = _env(B, A, servo=ready)
        assert owner.servo is ready
        owner.close()
    finally:
        env.close()


def test_step_outputs_is_refused_and_a_refused_step_pushes_no_frame():
    """``autograd.step_outputs`` differentiates with respect to the action it is given; with a servo the mirror receives another one, so it
    raises before anything is stepped (on an env without a servo it goes on working).  A ``step`` that raises on its ``out`` tensors has
    not moved the servo.  ``output_gradient(wrt="action")`` after a plain step is taken at what the mirror received."""
    torch = _torch()
    from adaptive_optics_gym_amd.autograd import step_outputs

    B, A = 3, 5
    env, bare = _env(B, A, servo=dict(latency=0.5, response=0.5)), _env(B, A)
    try:
        env.reset(), bare.reset()
        a = _acts(torch, B, A, 0)[1].requires_grad_(True)
        env.step(a.detach())
        blob, clock = env.servo.get_state(), (env.timestep, env.observation_frames, env.state_epoch)
        with pytest.raises(RuntimeError, match="mirror servo.*applied_action"):
            step_outputs(env, a)
        with pytest.raises(ValueError, match="out="):
            env.step(a.detach(), out=(torch.zeros(1, device="cuda"),) * 3)
        assert torch.equal(env.servo.get_state(), blob) and (env.timestep, env.observation_frames, env.state_epoch) == clock
        step_outputs(bare, a)[2].sum().backward()
        assert a.grad is not None and bool(torch.isfinite(a.grad).all()) and bool(a.grad.abs().sum() > 0)
        # the gradient after a plain step: at the applied action, not at the command
        b = _acts(torch, B, A, 1)[1]
        applied = env.step(b)[4]["applied_action"]
        assert not torch.equal(applied, b)
        one = torch.ones(B, dtype=torch.float64, device="cuda")
        got = env.output_gradient(g_strehl=one, wrt="action")
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, env.output_gradient(g_strehl=one, wrt="action", action=applied))
        assert not torch.equal(got, env.output_gradient(g_strehl=one, wrt="action", action=b))
    finally:
        env.close(), bare.close()


def test_layered_set_state_refuses_a_servo_mismatch_before_a_layer_is_touched():
    torch = _torch()
    from adaptive_optics_gym_amd import LayeredAOEnv

    B, A = 3, 5
    kw = dict(atm_layers=[{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}], atm_fried=0.15, seed=11, act_type="zernike", act_dim=A,
              obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=6, num_pupil_pixels=N, verbose=False)
    env, bare, deep = LayeredAOEnv(B, "cuda:0", servo=dict(latency=1), **kw), LayeredAOEnv(B, "cuda:0", **kw), LayeredAOEnv(B, "cuda:0", servo=dict(latency=3), **kw)
    try:
        for e in (env, bare, deep):
            e.reset()
        a = _acts(torch, B, A, 0)[1]
        env.step(a), env.step(a)
        snap = env.get_state()
        for other, word in ((bare, "mirror servo"), (deep, "another servo")):
            before = [lay.get_screens().clone() for lay in other.layers]
            with pytest.raises(ValueError, match=word):
                other.set_state(snap)
            assert all(torch.equal(x, lay.get_screens()) for x, lay in zip(before, other.layers)) and other.timestep == 0
        with pytest.raises(ValueError, match="mirror servo"):
            env.set_state(bare.get_state())
    finally:
        env.close(), bare.close(), deep.close()


def test_rollout_runs_its_unfused_loop_through_the_servo():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import rollout

    B, A, T = 3, 20, 5
    scr = smooth_screens(B, N, 5, amp=1e-5, sigma_frac=0.15)
    env = _env(B, A, T, "num_actuators", screens=scr, SH_operation=True, servo=dict(latency=1))
    twin = _env(B, A, T, "num_actuators", screens=scr, SH_operation=True)
    try:
        out = rollout(env, None, policy="ideal")
        # the same loop by hand on the servo-less twin: the mirror gets the command of one step earlier
        obs = twin.reset()[0]
        prev = torch.zeros((B, A), device="cuda")
        for t in range(T):
            cmd = twin.ideal_action().to(torch.float32)
            assert torch.equal(out["act"][t], cmd), f"step {t}: the stored action is the command"
            ret = twin.step(prev)
            assert torch.equal(out["next_obs"][t], ret[0]) and torch.equal(out["rew"][t], ret[1]), f"step {t}"
            prev = cmd
    finally:
        env.close(), twin.close()
