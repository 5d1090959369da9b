"""Residual wavefront statistics and the best-fit mirror command on the device (aog_wavefront_truth: k_wavefront_fit<A_PAD>, k_wavefront_ref,
k_wavefront_finish) against the host restatement tests/wavefront_reference.py, which builds the phase from get_screens(), get_actuators()
and env.tables.modes.  Shapes: N = 32 has 812 aperture pixels = 26 pixel tiles with 12 pixels in the last; B = 33 is two env tiles, the
second holding one env; the padded mode counts are 16 (zernike-6), 32 (20 modes), 64 (64 modes) and 128 (100 modes at N = 64, 51 pixel tiles).
N = 52 (EDGE, B = 40) has 2128 aperture pixels = 67 pixel tiles: the second chunk of 64 holds tiles 64 .. 66, so wave 3 of its workgroups
has no tile, and the last tile has 16 real pixels.
PARITY = 1e-5 is the project's standing bound for fast handles against float64, 1e-10 the float64 handles'.
Each figure is printed before it is asserted (run with -s); the measured maxima are in profiles/wavefront_truth.md."""
import ctypes as C

import numpy as np
import pytest

import wavefront_reference as wr
from helpers import actions_for, assert_short_last_chunk, smooth_screens

pytestmark = pytest.mark.gpu

N, B = 32, 33
PARITY, PARITY64 = 1e-5, 1e-10
KEYS = ("rms", "fit_rms", "coef", "ideal_actuators")
CASES = {"apad16": ("zernike", 6, 32), "apad32": ("num_actuators", 20, 32), "apad64": ("num_actuators", 64, 32), "apad128": ("num_actuators", 100, 64)}
EDGE, EDGE_B = ("num_actuators", 20, 52), 40   # a wave without tiles (not in CASES, which other files run in full)
assert_short_last_chunk(EDGE[2])
_TABLES = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(num_envs=B, act_type="num_actuators", act_dim=20, n=N, **kw):
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.optics_host import build_tables, obs_route_for
    from adaptive_optics_gym_amd.params import OpticalParams

    base = dict(obs_dim=2, timesteps_per_episode=4, seed=17, screen_oversampling=4, verbose=False)
    base.update(kw)
    key = (act_type, act_dim, n, base["obs_dim"], obs_route_for(base.get("precision", "fast"), base["obs_dim"]))
    if key not in _TABLES:   # the host precompute once per shape; every handle of that shape shares it
        _TABLES[key] = build_tables(OpticalParams(num_pupil_pixels=n), act_type, act_dim, base["obs_dim"], obs_route=key[4])
    return BatchedAOEnv(num_envs, "cuda:0", act_type=act_type, act_dim=act_dim, num_pupil_pixels=n, tables=_TABLES[key], **base)


def _hold(env, bound, what, vectors=("coef", "ideal_actuators")):
    """The device's four results against the host restatement of the env's current state: rms and fit_rms within bound x rms, coef and
    ideal_actuators within bound x their vector's largest magnitude, per env.  Returns (device results as numpy, host results)."""
    got = {k: v.cpu().numpy() for k, v in env.wavefront_truth().items()}
    ref = wr.host_truth(env)
    worst = {}
    for k in ("rms", "fit_rms"):
        worst[k] = float(np.max(np.abs(got[k] - ref[k]) / ref["rms"]))
    for k in vectors:
        scale = np.abs(ref[k]).max(axis=1)
        assert np.all(scale > 0), f"{what}: {k} of some env is identically zero: the case checks nothing"
        worst[k] = float(np.max(np.abs(got[k] - ref[k]).max(axis=1) / scale))
    print(f"{what}: max deviation / bound scale  " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"   (rms {ref['rms'].min():.3e} .. {ref['rms'].max():.3e} m, fit_rms / rms {np.min(ref['fit_rms'] / ref['rms']):.3f} .. {np.max(ref['fit_rms'] / ref['rms']):.3f})")
    for k, v in worst.items():
        assert v <= bound, f"{what}: {k} deviates {v:.3e} > {bound:g}"
    return got, ref


def _raw_actions(torch, num_envs, A, seed):
    """Raw actuator vectors (SH_operation=True) of ~50 nm per mode."""
    return torch.from_numpy(actions_for(num_envs, A, seed) * np.float32(5e-8)).cuda()


# ---- 1. parity with the host restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES) + ["edge52"])
@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_parity_with_the_host_restatement(case, precision):
    torch = _torch()
    act_type, A, n = CASES.get(case, EDGE)
    nb = EDGE_B if case == "edge52" else B
    bound = PARITY if precision == "fast" else PARITY64
    scr = smooth_screens(nb, n, 31)
    for raw in (True, False):
        # (the Shack-Hartmann chain, and with it SH_operation=True, is built for fast handles only: a float64 handle gets its raw actuator
        # vectors through set_actuators)
        env = _env(nb, act_type, A, n, screens=scr, SH_operation=raw and precision == "fast", precision=precision)
        try:
            env.reset()
            if raw:   # (once per case: the flat mirror)
                _hold(env, bound, f"{case} {precision} after reset")
            if raw and precision == "fp64":
                env.set_actuators(_raw_actions(torch, nb, A, 1).to(torch.float64))
            else:
                for t in range(2):
                    env.step(_raw_actions(torch, nb, A, t) if raw else torch.from_numpy(actions_for(nb, A, t)).cuda())
            _hold(env, bound, f"{case} {precision}, {'raw actuators' if raw else 'two steps of normalised actions'}")
        finally:
            env.close()


# ---- 2. closing the loop -------------------------------------------------------------------------------------------------------------------
def test_stepping_the_ideal_action_leaves_the_fitting_error():
    """Screens smooth and weak enough (0.2 um rms of path: half a radian at the science wavelength) that the Strehl ratio falls with the
    residual variance, which the fit cannot raise."""
    torch = _torch()
    env = _env(B, "num_actuators", 20, screens=smooth_screens(B, N, 5, amp=1e-5, sigma_frac=0.15), SH_operation=True)
    try:
        env.reset()
        flat = env.step(torch.zeros((B, 20), dtype=torch.float32, device="cuda:0"))
        strehl_flat = flat[4]["strehl"].clone()
        before, _ = _hold(env, PARITY, "flat mirror")
        ideal = env.ideal_action()
        assert torch.equal(ideal, env.wavefront_truth()["ideal_actuators"])
        stepped = env.step(ideal.to(torch.float32))
        # (coef of the fitted state is zero up to rounding and has no magnitude of its own to be held against: it is held through
        # ideal_actuators = actuators - coef / 2, at the actuators' magnitude)
        after, _ = _hold(env, PARITY, "after stepping the ideal action", vectors=("ideal_actuators",))
        on_mirror = env.get_actuators().cpu().numpy()
        d_rms = np.abs(after["rms"] - before["fit_rms"]) / before["rms"]
        d_act = np.abs(after["ideal_actuators"] - on_mirror).max(axis=1) / np.abs(on_mirror).max(axis=1)
        gain = (stepped[4]["strehl"] - strehl_flat).cpu().numpy()
        print(f"new rms against old fit_rms, / old rms: {d_rms.max():.2e};  new ideal actuators against the mirror's: {d_act.max():.2e};  "
              f"Strehl {float(strehl_flat.min()):.3f} .. {float(strehl_flat.max()):.3f} -> {float(stepped[4]['strehl'].min()):.3f} .. "
              f"{float(stepped[4]['strehl'].max()):.3f}, smallest gain {gain.min():.3e}")
        # (the action is rounded to float32 on its way in: 6e-8 of the actuators, far inside the bound)
        assert d_rms.max() <= PARITY and d_act.max() <= PARITY
        assert np.all(gain > 0)
    finally:
        env.close()


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(atm_type="quasi_static"), dict(atm_type="dynamic", atm_vel=20.0)], ids=["quasi_static", "dynamic_int8_work_ahead"])
def test_nothing_a_step_reads_or_writes_moves(kw):
    torch = _torch()
    A, T = 20, 4
    env, twin = _env(B, act_dim=A, **kw), _env(B, act_dim=A, **kw)
    try:
        o1, _ = env.reset()
        o2, _ = twin.reset()
        assert torch.equal(o1, o2)
        for t in range(T):
            truth = env.wavefront_truth()   # between every two steps of the episode
            assert all(bool(torch.isfinite(v).all()) for v in truth.values())
            a = torch.from_numpy(actions_for(B, A, t)).cuda()
            r1, r2 = env.step(a), twin.step(a)
            for k, name in ((0, "obs"), (1, "reward"), (2, "done")):
                assert torch.equal(r1[k], r2[k]), f"step {t}: {name} moved"
            for k in ("power", "strehl", "obs_raw"):
                assert torch.equal(r1[4][k], r2[4][k]), f"step {t}: {k} moved"
            assert torch.equal(env.get_actuators(), twin.get_actuators()), f"step {t}: the mirror moved"
        env.wavefront_truth()
        if env.atm_type == "dynamic":
            assert env.extrusion_kmax > 0   # (the int8 extrusion, whose work ahead the call must leave alone)
            assert torch.equal(env.get_screens(), twin.get_screens())
        assert env.device_status() == 0
    finally:
        env.close()
        twin.close()


# ---- 4. a split batch reproduces the whole one ----------------------------------------------------------------------------------------------
def test_split_batch_is_bit_identical():
    torch = _torch()
    A = 20
    whole = _env(B, act_dim=A, total_envs=B)
    parts = [_env(16, act_dim=A, global_env_offset=0, total_envs=B), _env(17, act_dim=A, global_env_offset=16, total_envs=B)]
    try:
        a = torch.from_numpy(actions_for(B, A, 3)).cuda()
        whole.reset()
        whole.step(a)
        ref = whole.wavefront_truth()
        got = []
        for env, sl in zip(parts, (slice(0, 16), slice(16, 33))):
            env.reset()
            env.step(a[sl].contiguous())
            got.append(env.wavefront_truth())
        for k in KEYS:
            assert torch.equal(torch.cat([g[k] for g in got]), ref[k]), f"{k}: 16 + 17 envs differ from 33"
        assert float(ref["rms"].min()) > 0
    finally:
        for env in [whole] + parts:
            env.close()


# ---- 5. dynamic atmosphere -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_dynamic_parity(extrusion):
    torch = _torch()
    A = 20
    env = _env(B, act_dim=A, atm_type="dynamic", atm_vel=20.0, extrusion=extrusion)
    try:
        env.reset()
        for t in range(3):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
            _hold(env, PARITY, f"dynamic, extrusion={extrusion}, step {t + 1}")
    finally:
        env.close()


# ---- 6. guards -----------------------------------------------------------------------------------------------------------------------------
def test_guards():
    torch = _torch()
    from adaptive_optics_gym_amd import _lib
    from adaptive_optics_gym_amd.rollout import DeviceActor, make_actor

    A = 20
    env = _env(B, act_dim=A, timesteps_per_episode=3)
    try:
        env.reset()
        ok = env.wavefront_truth()
        # an action pending after a pipelined step
        a = [torch.from_numpy(actions_for(B, A, t)).cuda() for t in range(2)]
        env.step(a[0], next_actions=a[1])
        with pytest.raises(RuntimeError, match="aog_wavefront_truth"):
            env.wavefront_truth()
        env.step(a[1], next_actions=None)
        env.wavefront_truth()
        # ... and after reset_with_policy, until the episode's last step has queried nothing
        actor = make_actor(4, A, 16, device="cuda:0")
        pol = DeviceActor(actor, seed=1, env_id_base=0)
        env.reset_with_policy(pol)
        with pytest.raises(RuntimeError, match="aog_wavefront_truth"):
            env.wavefront_truth()
        for t in range(3):
            _, queried = env.step_with_policy(pol)
            if queried is not None:
                with pytest.raises(RuntimeError, match="aog_wavefront_truth"):
                    env.wavefront_truth()
        assert queried is None
        env.wavefront_truth()
        # new tables invalidate the fit; the binding uploads it again
        env.reset()
        env._upload_tables()
        out = torch.empty((B,), dtype=torch.float64, device="cuda:0")
        rc = env.lib.aog_wavefront_truth(env._handle, C.c_void_p(out.data_ptr()), None, None, None, env._stream())
        assert rc == -3 and b"aog_upload_wavefront_fit" in env.lib.aog_last_error()   # AOG_ERR_STATE
        with pytest.raises(RuntimeError):
            _lib.check(rc)
        again = env.wavefront_truth()
        for k in KEYS:
            assert torch.equal(again[k], ok[k]), k
    finally:
        env.close()
    # between two steps of a lookahead episode
    env = _env(B, act_dim=A, atm_type="dynamic", atm_vel=20.0, timesteps_per_episode=3)
    try:
        assert env.lookahead(True)
        env.reset()
        env.wavefront_truth()
        for t in range(3):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
            if t < 2:
                with pytest.raises(RuntimeError, match="aog_wavefront_truth"):
                    env.wavefront_truth()
        env.wavefront_truth()   # the episode's last step never looks ahead
        env.lookahead(False)
    finally:
        env.close()


# ---- 7. the ideal modal controller in a rollout --------------------------------------------------------------------------------------------
def test_rollout_with_the_ideal_policy():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import rollout

    A, T = 20, 3
    scr = smooth_screens(B, N, 8)
    env = _env(B, act_dim=A, screens=scr, SH_operation=True, timesteps_per_episode=T)
    twin = _env(B, act_dim=A, screens=scr, SH_operation=True, timesteps_per_episode=T)
    flat = _env(B, act_dim=A, screens=scr, SH_operation=False, timesteps_per_episode=T)
    try:
        out = rollout(env, None, episodes=1, policy="ideal")
        assert tuple(out["act"].shape) == (T, B, A) and bool((out["log_prob"] == 1).all())
        twin.reset()
        for t in range(T):
            a = twin.ideal_action().to(torch.float32)   # from the state the last observation saw, applied to the next screen
            assert torch.equal(out["act"][t], a), f"step {t}: the rollout's action is not ideal_action()"
            r = twin.step(a)
            assert torch.equal(out["next_obs"][t], r[0]) and torch.equal(out["rew"][t], r[1])
        assert float(out["act"][0].abs().max()) > 0
        with pytest.raises(ValueError, match="SH_operation=True"):
            rollout(flat, None, episodes=1, policy="ideal")
        for bad in (dict(action_mode="mean"), dict(fused_policy=True)):
            with pytest.raises(ValueError):
                rollout(env, None, episodes=1, policy="ideal", **bad)
    finally:
        for e in (env, twin, flat):
            e.close()
