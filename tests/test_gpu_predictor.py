"""The predictive controller on the device: aog_predictor_update (csrc/k_predictor.h) against the numpy restatement of its recursion
(tests/predictor_reference.py), its bit-for-bit properties (split batch, masks, warm-up, non-finite rows, reset, checkpoint) and the closed
loop through ``PredictiveController`` and ``rollout(policy="predictive")``.

Tolerance of every comparison with the reference: per shape and per quantity, the largest difference between the float64 and the longdouble
run of the reference relative to max |quantity| (the envelope: what float64 rounding alone does to this recursion on this input); the device
may differ from the float64 reference by 8 x that — it adds the dot products in another order, nothing else."""
import math

import numpy as np
import pytest

from predictor_reference import RLSReference, rel_diff, run, var1_sequence

pytestmark = pytest.mark.gpu

FACTOR = 8.0
LAM, P0, SCALE = 0.999, 1e3, 1.5e-6 / (2 * math.pi)
# (B, A, order): n = 5; 21 (no power of two, below a wave); 48; 256 (the limit, two-read form); 66 (A just over a half-wave, two column blocks)
SHAPES = [(3, 5, 1), (4, 7, 3), (5, 16, 3), (2, 64, 4), (2, 33, 2)]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _dev(B, A, order, lam=LAM, p0=P0, scale=SCALE):
    from adaptive_optics_gym_amd.predictor import DevicePredictor

    return DevicePredictor(B, A, order, lam, p0, scale, device="cuda:0")


def _feed(torch, dev, ys, masks=None, fill=None):
    """Feed ys [T, B, A] to a device handle; (pred, innov) [T, B, A] numpy.  Rows a mask leaves out keep ``fill`` (they are not written)."""
    preds, innovs = [], []
    for t, y in enumerate(ys):
        yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        out = None
        if fill is not None:
            out = (torch.full_like(yt, fill), torch.full_like(yt, fill))
        p, i = dev.update(yt, None if masks is None else masks[t], out=out)
        preds.append(p.cpu().numpy())
        innovs.append(i.cpu().numpy())
    return np.stack(preds), np.stack(innovs)


def _blob_equal(torch, a, b):
    return all(torch.equal(a[k], b[k]) for k in ("W", "P", "history", "count", "skipped"))


def _envelope_check(label, dev_q, f64_q, ld_q):
    """Print and assert the 8 x envelope bound for the quantities (pred, innov, W, P); returns the figures."""
    figs = []
    for name, d, f, l in zip(("pred", "innov", "W", "P"), dev_q, f64_q, ld_q):
        env, got = rel_diff(f, l), rel_diff(d, f)
        figs.append((env, got))
        print(f"{label} {name}: envelope {env:.3e}  device {got:.3e}  ({got / env if env else 0:.2f} x)")
    for (env, got) in figs:
        assert env < 1e-6, "the recursion is ill-conditioned on this input: shorten T or raise lam, do not widen the factor"
        assert got <= FACTOR * env
    return figs


# ---- 1. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,order", SHAPES, ids=[f"B{b}_A{a}_p{p}" for b, a, p in SHAPES])
def test_replay_against_the_reference(B, A, order):
    torch = _torch()
    n = A * order
    T = 3 * n + 10
    ys = var1_sequence(100 + n, T, B, A)
    refs = {}
    for name, dt in (("f64", np.float64), ("ld", np.longdouble)):
        r = RLSReference(B, A, order, LAM, P0, SCALE, dt)
        refs[name] = run(r, ys) + (r.W, r.P)
    dev = _dev(B, A, order)
    pred, innov = _feed(torch, dev, ys)
    st = dev.unpack()
    assert np.array_equal(pred[:order], ys[:order]) and not innov[:order].any()
    assert st["count"].tolist() == [T] * B and st["skipped"].tolist() == [0] * B
    P = st["P"].cpu().numpy()
    assert np.array_equal(P, P.transpose(0, 2, 1))   # symmetric bit for bit
    _envelope_check(f"replay B={B} A={A} order={order} n={n} T={T}", (pred, innov, st["W"].cpu().numpy(), P), refs["f64"], refs["ld"])
    dev.close()


# ---- 2. split equals whole ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,order", [(7, 3), (33, 2), (40, 4)], ids=["n21", "n66", "n160_two_read"])
def test_split_batch_equals_whole_batch(A, order):
    torch = _torch()
    T = 2 * order + 12
    ys = var1_sequence(7, T, 5, A)
    whole, lo, hi = _dev(5, A, order), _dev(2, A, order), _dev(3, A, order)
    pw, iw = _feed(torch, whole, ys)
    pl, il = _feed(torch, lo, ys[:, :2])
    ph, ih = _feed(torch, hi, ys[:, 2:])
    assert np.array_equal(pw, np.concatenate([pl, ph], axis=1)) and np.array_equal(iw, np.concatenate([il, ih], axis=1))
    assert torch.equal(whole.get_state(), torch.cat([lo.get_state(), hi.get_state()]))
    assert iw[order:].any()
    for d in (whole, lo, hi):
        d.close()


# ---- 3. masks ----------------------------------------------------------------------------------------------------------------------------
def test_masked_updates_touch_only_the_selected_envs():
    torch = _torch()
    B, A, order, T = 4, 9, 2, 10
    ys = var1_sequence(21, T, B, A)
    masks = [np.array([(t + b) % 2 == 0 for b in range(B)]) for t in range(T)]   # alternate
    dev = _dev(B, A, order)
    twins = [_dev(1, A, order) for _ in range(B)]
    for t in range(T):
        before = dev.unpack()
        pred, innov = _feed(torch, dev, ys[t:t + 1], [masks[t]], fill=-7.0)
        after = dev.unpack()
        for b in range(B):
            if masks[t][b]:
                tp, ti = _feed(torch, twins[b], ys[t:t + 1, b:b + 1])
                assert np.array_equal(pred[0, b], tp[0, 0]) and np.array_equal(innov[0, b], ti[0, 0])
            else:   # state and output rows unchanged bitwise
                assert all(torch.equal(before[k][b], after[k][b]) for k in before)
                assert (pred[0, b] == -7.0).all() and (innov[0, b] == -7.0).all()
    assert torch.equal(dev.get_state(), torch.cat([tw.get_state() for tw in twins]))
    for d in [dev] + twins:
        d.close()


# ---- 4. warm-up, non-finite input, reset -------------------------------------------------------------------------------------------------
def test_warm_up_non_finite_rows_and_reset():
    torch = _torch()
    B, A, order, T = 3, 6, 3, 12
    ys = var1_sequence(33, T, B, A)
    dev, clean = _dev(B, A, order), _dev(B, A, order)
    fresh = dev.unpack()
    assert fresh["count"].tolist() == [0] * B and torch.equal(fresh["P"][0], P0 * torch.eye(A * order, dtype=torch.float64, device="cuda"))
    assert torch.equal(fresh["W"][0], torch.eye(A * order, dtype=torch.float64, device="cuda")[:, :A]) and not fresh["history"].any()
    pred, innov = _feed(torch, dev, ys[:6])
    _feed(torch, clean, ys[:6])
    assert np.array_equal(pred[:order], ys[:order]) and not innov[:order].any()   # the first `order` predictions are the measurements
    assert not np.array_equal(pred[order], ys[order]) and innov[order].any()
    # a NaN (then an inf) in env 1's row: its state stays bit for bit, its pred row is its y row, skipped counts, the neighbours go on
    for k, poison in enumerate((np.nan, -np.inf)):
        before = dev.unpack()
        bad = ys[6 + k].copy()
        bad[1, 2] = poison
        p, i = _feed(torch, dev, bad[None])
        pc, ic = _feed(torch, clean, ys[6 + k][None], [np.array([True, False, True])])
        after = dev.unpack()
        assert np.array_equal(p[0, 1], bad[1], equal_nan=True) and not i[0, 1].any()
        assert all(torch.equal(before[key][1], after[key][1]) for key in ("W", "P", "history", "count"))
        assert after["skipped"].tolist() == [0, k + 1, 0]
        assert np.array_equal(p[0, [0, 2]], pc[0, [0, 2]]) and np.array_equal(i[0, [0, 2]], ic[0, [0, 2]])
    # reset(mask): env 1 back to the initial state, the others untouched
    before = dev.unpack()
    dev.reset(np.array([False, True, False]))
    after = dev.unpack()
    assert all(torch.equal(after[key][1], fresh[key][1]) for key in fresh)
    assert all(torch.equal(after[key][[0, 2]], before[key][[0, 2]]) for key in fresh)
    p, i = _feed(torch, dev, ys[8:8 + order])
    assert np.array_equal(p[:, 1], ys[8:8 + order, 1]) and not i[:, 1].any() and i[:, 0].all()
    dev.reset()
    assert _blob_equal(torch, dev.unpack(), fresh)
    dev.close()
    clean.close()


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,order", [(16, 3), (40, 4)], ids=["register_form", "two_read_form"])
def test_checkpoint_resumes_bit_identically(A, order):
    torch = _torch()
    B, k, T = 3, order + 4, order + 10
    ys = var1_sequence(44, T, B, A)
    straight, first, second = _dev(B, A, order), _dev(B, A, order), _dev(B, A, order)
    ps, is_ = _feed(torch, straight, ys)
    _feed(torch, first, ys[:k])
    blob = first.get_state()
    assert blob.numel() == B * 8 * (A * order * A + (A * order) ** 2 + A * order + 2)
    second.set_state(blob)
    p2, i2 = _feed(torch, second, ys[k:])
    assert np.array_equal(ps[k:], p2) and np.array_equal(is_[k:], i2)
    assert torch.equal(straight.get_state(), second.get_state())
    with pytest.raises(ValueError, match="blob"):
        second.set_state(blob[:-8])
    for d in (straight, first, second):
        d.close()


# ---- 6. closed loop ----------------------------------------------------------------------------------------------------------------------
N_PUPIL, ACT, ORDER, WIND = 32, 16, 2, 30.0   # the smallest pupil of the GPU tests; 30 m/s moves the screen two pixels per step
STEPS = 10 * ACT * ORDER


def _recording(ctrl):
    """Wrap ctrl.update so that every measurement, prediction and innovation of the loop is kept in float64."""
    ys, preds, innovs, inner = [], [], [], ctrl.update

    def update(y, mask=None):
        pred = inner(y, mask)
        ys.append(y.clone())
        preds.append(pred.clone())
        innovs.append(ctrl.innovation.clone())
        return pred

    ctrl.update = update
    return ys, preds, innovs


def _closed_loop(torch, env, label):
    from adaptive_optics_gym_amd.predictor import PredictiveController
    from adaptive_optics_gym_amd.rollout import rollout

    B, A = env.num_envs, env.num_modes
    ctrl = PredictiveController(env, order=ORDER, measurement="truth")
    assert ctrl.scale == env.wavelength_wfs / (2 * math.pi) and ctrl.forgetting == 0.999 and ctrl.p0 == 1e3
    ys, preds, innovs = _recording(ctrl)
    out = rollout(env, None, episodes=1, policy="predictive", predictor=ctrl)
    ys, preds, innovs = (torch.stack(v).cpu().numpy() for v in (ys, preds, innovs))
    T = len(ys)
    assert T == STEPS and out["act"].shape == (T, B, A) and bool((out["log_prob"] == 1).all())
    assert torch.equal(out["act"].cpu(), torch.from_numpy(preds).float())
    assert ctrl.innovation is not None and tuple(ctrl.innovation.shape) == (B, A)
    refs = {}
    for name, dt in (("f64", np.float64), ("ld", np.longdouble)):
        r = RLSReference(B, A, ORDER, ctrl.forgetting, ctrl.p0, ctrl.scale, dt)
        refs[name] = run(r, ys) + (r.W, r.P)
    st = ctrl.predictor.unpack()
    figs = _envelope_check(label, (preds, innovs, st["W"].cpu().numpy(), st["P"].cpu().numpy()), refs["f64"], refs["ld"])
    ctrl.close()
    return out, ys, preds, refs, figs


def _energy_ratio(ys, preds):
    """sum |y_{t+1} - pred_t|^2 over sum |y_{t+1} - y_t|^2 (what 'ideal' commits) over the second half of the run."""
    h = len(ys) // 2
    return float(((ys[h + 1:] - preds[h:-1]) ** 2).sum() / ((ys[h + 1:] - ys[h:-1]) ** 2).sum())


def test_closed_loop_recovers_the_servo_lag():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.predictor import PredictiveController
    from adaptive_optics_gym_amd.rollout import rollout

    kw = dict(atm_type="dynamic", atm_vel=WIND, SH_operation=True, act_dim=ACT, obs_dim=2, num_pupil_pixels=N_PUPIL, timesteps_per_episode=STEPS,
              rew_type="strehl_ratio", seed=17, verbose=False)   # (the reward is a function of the Strehl ratio: what the last lines report)
    env = BatchedAOEnv(4, "cuda:0", **kw)
    shift = WIND * env.delta_t / env.params.pupil_pixel
    assert shift >= 1.0, shift
    out, ys, preds, refs, figs = _closed_loop(torch, env, f"closed loop N={N_PUPIL} wind={WIND} ({shift:.2f} px/step)")
    got, want = _energy_ratio(ys, preds), _energy_ratio(ys, np.asarray(refs["f64"][0], np.float64))
    # what the replay tolerance allows the ratio: every prediction within tol = 8 x envelope x max |pred| of the reference's moves the error
    # energy E = sum (y - pred)^2 over M entries by at most 2 sqrt(E M) tol + M tol^2 (Cauchy-Schwarz), and the ratio by that over the
    # persistence energy
    h = len(ys) // 2
    M = ys[h + 1:].size
    tol = FACTOR * figs[0][0] * np.abs(refs["f64"][0]).max()
    pers = float(((ys[h + 1:] - ys[h:-1]) ** 2).sum())
    allowed = (2.0 * math.sqrt(want * pers * M) * tol + M * tol * tol) / pers
    print(f"closed loop: prediction / persistence energy, second half: device {got:.9f}, float64 reference {want:.9f}, "
          f"difference {abs(got - want):.3e} of {allowed:.3e} allowed")
    assert got < 1.0 and want < 1.0
    assert abs(got - want) <= allowed
    # refusals: an action pending; a measurement the env does not have
    ctrl = PredictiveController(env, order=1)
    env.reset()
    a = out["act"][0]
    env.step(a, next_actions=a)
    with pytest.raises(ValueError, match="pending|NEXT action"):
        ctrl.action()
    env.step(a, next_actions=None)
    ctrl.action()
    with pytest.raises(ValueError, match="pyramid=dict"):
        PredictiveController(env, measurement="pyramid")
    with pytest.raises(ValueError, match="another env"):
        rollout(env, None, policy="predictive", predictor=type("P", (), {"env": None})())
    ctrl.close()
    to_strehl = lambda rew: 1.0 + float(rew[STEPS // 2:].mean()) / 100.0   # (AO_env.py:479-483: reward = -(100 - Strehl in per cent), no threshold)
    strehl = {"predictive": to_strehl(out["rew"])}
    env.close()
    ideal = BatchedAOEnv(4, "cuda:0", **kw)
    strehl["ideal"] = to_strehl(rollout(ideal, None, episodes=1, policy="ideal")["rew"])
    ideal.close()
    print(f"closed loop: mean Strehl over the second half (not asserted): {strehl}")


def test_closed_loop_replay_on_a_two_layer_atmosphere():
    torch = _torch()
    from adaptive_optics_gym_amd import LayeredAOEnv

    env = LayeredAOEnv(4, "cuda:0", atm_layers=[dict(fraction=0.6, speed=20.0), dict(fraction=0.4, speed=45.0)], SH_operation=True, act_dim=ACT,
                       obs_dim=2, num_pupil_pixels=N_PUPIL, timesteps_per_episode=STEPS, seed=5, verbose=False)
    _, ys, preds, _, _ = _closed_loop(torch, env, "closed loop, two layers")
    print(f"two layers: prediction / persistence energy, second half (not asserted): {_energy_ratio(ys, preds):.6f}")
    env.close()


def test_pyramid_measurement_is_the_integrator_at_gain_one():
    torch = _torch()
    import ctypes as C

    from adaptive_optics_gym_amd import BatchedAOEnv, _lib
    from adaptive_optics_gym_amd.predictor import PredictiveController
    from adaptive_optics_gym_amd.rollout import rollout
    from helpers import smooth_screens

    B, N, A, T = 3, 64, 16, 4
    env = BatchedAOEnv(B, "cuda:0", act_dim=A, obs_dim=2, num_pupil_pixels=N, screens=smooth_screens(B, N, 31, amp=4e-6), SH_operation=True,
                       pyramid=dict(samples=16, pixels=16, n_mod=4, r_mod=2.0), timesteps_per_episode=T, verbose=False)
    ctrl = PredictiveController(env, order=1, measurement="pyramid")
    ys, preds, _ = _recording(ctrl)
    out = rollout(env, None, episodes=1, policy="predictive", predictor=ctrl)
    assert len(ys) == T and torch.equal(out["act"][0], ys[0].float())
    act = ctrl.action()                       # one more, at the state the last step left ...
    direct = torch.empty((B, A), dtype=torch.float64, device="cuda")
    frames = env.pyramid_frame_count
    _lib.check(env.lib.aog_pyramid_update(env._handle, 1.0, C.c_void_p(direct.data_ptr()), None, env._stream()))   # ... and the library's own
    assert torch.equal(ys[-1], direct) and torch.equal(ctrl.measurement_value, direct) and frames == T + 1
    assert act.dtype == torch.float64 and tuple(act.shape) == (B, A) and bool(torch.isfinite(act).all())
    ctrl.close()
    env.close()
