"""Observation grids up to 32 x 32 on the device (run with -m gpu on an MI355X): the separable route (fast handles with obs_dim >= 6, float64
handles with obs_dim >= 8) against the CPU oracle, fast against float64 on the same screens, under a dynamic atmosphere, pipelined stepping,
lookahead, state save / restore, the Shack-Hartmann chain, the rollout and the gym shim; the sizes below it keep the table route.

Tolerances as the other parity tests: observations before the float16 cast within 1e-5 relative (elements below 1e-3 of their vector's peak
held to the same absolute error), after the cast 1 float16 ulp, power / Strehl 1e-5, `done` exact."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from helpers import ScriptedRNG, actions_for, device_mode_stencil_draws, run_oracle, smooth_screens

pytestmark = pytest.mark.gpu

RTOL = 1e-5
LAM_WFS = 1.5e-6
KERNELS = [("fast", "mfma"), ("fast", "valu"), ("fp64", "auto")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _obs_close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    peak = ref.max(axis=-1, keepdims=True)
    bad = np.abs(got - ref) > RTOL * np.maximum(np.abs(ref), 1e-3 * peak)
    assert not bad.any(), f"max rel err {np.max(np.abs(got - ref) / np.abs(ref)):.3e}, {bad.sum()} elements out of tolerance"


def _ulp16_close(a, b):
    a = np.asarray(a, dtype=np.float16).view(np.int16).astype(np.int32)
    b = np.asarray(b, dtype=np.float16).view(np.int16).astype(np.int32)
    return np.all(np.abs(a - b) <= 1)


def _separable(env):
    return bool(env.info.reserved & 2)


def _drive(env, acts, torch):
    out = {k: [] for k in ("obs_raw", "obs", "reward", "done", "power", "strehl")}
    env.reset()
    obs0 = env.last_obs_raw.cpu().numpy().astype(np.float64)
    for t in range(acts.shape[0]):
        obs, r, d, _, info = env.step(torch.from_numpy(acts[t]).to(env.device))
        out["obs_raw"].append(info["obs_raw"].cpu().numpy().astype(np.float64))
        out["obs"].append(obs.cpu().numpy())
        out["reward"].append(r.cpu().numpy().astype(np.float64))
        out["done"].append(d.cpu().numpy())
        out["power"].append(info["power"].cpu().numpy().astype(np.float64))
        out["strehl"].append(info["strehl"].cpu().numpy().astype(np.float64))
        if bool(d.all()):
            env.reset()
    res = {k: np.stack(v) for k, v in out.items()}
    res["obs0"] = obs0
    return res


def _compare(got, ref, strehl_reward):
    _obs_close(got["obs0"], ref["obs0"])
    _obs_close(got["obs_raw"], ref["obs_raw"])
    assert _ulp16_close(got["obs"], ref["obs"])
    np.testing.assert_allclose(got["power"], ref["power"], rtol=RTOL)
    np.testing.assert_array_equal(got["done"], ref["done"].astype(bool))
    if strehl_reward:
        np.testing.assert_allclose(got["strehl"], ref["strehl"], rtol=RTOL)
        np.testing.assert_allclose(got["reward"], ref["reward"], rtol=0, atol=100 * RTOL)
    else:
        np.testing.assert_allclose(got["reward"], ref["reward"], rtol=RTOL, atol=1e-7)


@pytest.mark.parametrize("precision,kernel", KERNELS)
@pytest.mark.parametrize("N,B,A,o,act_type,rew", [
    (64, 37, 16, 6, "num_actuators", "strehl_ratio"),
    (64, 5, 6, 8, "zernike", "smf_ssim"),
    (96, 3, 64, 11, "num_actuators", "smf_ssim"),
    (240, 2, 64, 16, "num_actuators", "strehl_ratio"),
    (256, 33, 64, 32, "num_actuators", "smf_ssim"),
    (128, 1, 6, 16, "zernike", "strehl_ratio"),
])
def test_live_oracle_parity_obs_grid(N, B, A, o, act_type, rew, precision, kernel):
    """Reset and three steps across an episode end against the oracle (up to three envs of the batch)."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    T = 3
    scr = smooth_screens(B, N, seed=N + B + o)
    acts = np.stack([actions_for(B, A, 7 * s + N + o) for s in range(T)])
    kw = dict(act_type=act_type, act_dim=A, obs_dim=o, rew_type=rew, timesteps_per_episode=2)
    nb = min(B, 3)
    ref = run_oracle(scr[:nb], acts[:, :nb], **kw)
    env = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, screens=scr, precision=precision, kernel=kernel, verbose=False, **kw)
    assert _separable(env) == (o > (7 if precision == "fp64" else 5))
    got = _drive(env, acts, torch)
    assert got["obs_raw"].shape == (T, B, o * o)
    got = {k: (v[:, :nb] if k != "obs0" else v[:nb]) for k, v in got.items()}
    _compare(got, ref, rew == "strehl_ratio")
    env.close()


def test_fast_against_fp64_o16(record_property):
    """B = 256, N = 256, o = 16, one 20-step episode on the same screens and actions: the matrix-core route against the float64 one."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A, o, T = 256, 256, 64, 16, 20
    kw = dict(act_dim=A, obs_dim=o, timesteps_per_episode=T, num_pupil_pixels=N, verbose=False)
    fast = BatchedAOEnv(B, "cuda:0", seed=3, screen_source="device", **kw)
    ref = BatchedAOEnv(B, "cuda:0", screens=fast.get_screens(), precision="fp64", **kw)
    assert _separable(fast) and _separable(ref)
    fast.reset()
    ref.reset()
    _obs_close(fast.last_obs_raw.double().cpu().numpy(), ref.last_obs_raw.double().cpu().numpy())
    gen = torch.Generator("cuda").manual_seed(11)
    faint_worst, worst = 0.0, 0.0
    for t in range(T):
        a = 0.3 * torch.randn((B, A), device="cuda", generator=gen)
        o1, r1, d1, _, i1 = fast.step(a)
        o2, r2, d2, _, i2 = ref.step(a)
        got, want = i1["obs_raw"].double().cpu().numpy(), i2["obs_raw"].double().cpu().numpy()
        _obs_close(got, want)
        assert _ulp16_close(o1.cpu().numpy(), o2.cpu().numpy())
        np.testing.assert_allclose(i1["power"].cpu().numpy(), i2["power"].cpu().numpy(), rtol=RTOL)
        # (the Strehl ratio comes from the unchanged table kernels; a few envs of these device screens sit near 1e-5, where the obs rule's
        # absolute floor — 1e-5 x 1e-3 of the largest possible value, 1 — applies)
        np.testing.assert_allclose(i1["strehl"].cpu().numpy(), i2["strehl"].cpu().numpy(), rtol=RTOL, atol=1e-8)
        assert torch.equal(d1, d2)
        rel = np.abs(got - want) / np.abs(want)
        faint = want < 1e-3 * want.max(axis=1, keepdims=True)
        worst = max(worst, float(rel[~faint].max()))
        if faint.any():
            faint_worst = max(faint_worst, float(rel[faint].max()))
    record_property("max_rel_err", worst)
    record_property("max_rel_err_faint", faint_worst)
    print(f"fast vs fp64, o = 16, N = 256: worst relative error {worst:.2e} (pixels >= 1e-3 of the peak), {faint_worst:.2e} (fainter pixels)")
    fast.close()
    ref.close()


def test_dynamic_o8_int8_f64_and_oracle(record_property):
    """Dynamic atmosphere at o = 8 (separable on fast handles), one 30-step episode: the int8 composite extrusion against extrusion='f64' on
    the same device stream, and against the oracle's InfiniteAtmosphericLayer with the normals replayed."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.atmosphere_host import integer_shifts
    from oracle.ao_env_oracle import AOEnvOracle

    B, N, A, o, T, seed = 48, 128, 16, 8, 30, 9
    kw = dict(atm_type="dynamic", atm_vel=10, atm_fried=0.15, act_type="num_actuators", act_dim=A, obs_dim=o, timesteps_per_episode=T)
    e8 = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, seed=seed, screen_source="device", screen_oversampling=4, verbose=False, **kw)
    e64 = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, seed=seed, screen_source="device", screen_oversampling=4, verbose=False,
                       extrusion="f64", **kw)
    assert _separable(e8) and e8.extrusion_kmax >= 1 and e64.extrusion_kmax == 0
    geo = device_mode_stencil_draws(seed, B, N)
    ids = [0, 23, B - 1]
    refs = {b: AOEnvOracle(num_pupil_pixels=N, screen=e8.get_screens(b, 1)[0].cpu().numpy().ravel(),
                           rng=ScriptedRNG(e8.wind_u[b], [g.copy() for g in geo]), verbose=False, **kw) for b in ids}
    e8.reset()
    e64.reset()
    for b in ids:
        refs[b].reset()
        _obs_close(e8.last_obs_raw[b].double().cpu().numpy(), refs[b].last_obs_raw)
    gen = torch.Generator("cuda").manual_seed(5)
    for t in range(T):
        a = torch.randn((B, A), device="cuda", generator=gen)
        counts = np.abs(integer_shifts(e8.velocity_vectors, e8.timestep * e8.delta_t, (e8.timestep + 1) * e8.delta_t,
                                       e8.params.pupil_pixel)).sum(axis=1)
        noise = torch.randn((B, max(int(counts.max()), 1), N), device="cuda", dtype=torch.float64, generator=gen)
        e8.set_extrusion_noise(noise)
        e64.set_extrusion_noise(noise)
        _, _, done, _, info = e8.step(a)
        _, _, _, _, info64 = e64.step(a)
        _obs_close(info["obs_raw"].double().cpu().numpy(), info64["obs_raw"].double().cpu().numpy())
        np.testing.assert_allclose(info["power"].cpu().numpy(), info64["power"].cpu().numpy(), rtol=RTOL)
        for b in ids:
            refs[b].rng.normals.extend(noise[b, :int(counts[b])].cpu().numpy())
            _, _, r_done, _, r_info = refs[b].step(a[b].cpu().numpy())
            _obs_close(info["obs_raw"][b].double().cpu().numpy(), refs[b].last_obs_raw)
            np.testing.assert_allclose(float(info["strehl"][b]), refs[b].last_strehl, rtol=RTOL)
            np.testing.assert_allclose(float(info["power"][b]), r_info["power"], rtol=RTOL)
            assert bool(done[b]) == r_done
    assert e8.device_status() == 0 and e64.device_status() == 0
    e8.close()
    e64.close()


@pytest.mark.parametrize("atm", ["quasi_static", "dynamic"])
def test_pipelined_stepping_bit_identical_o16(atm):
    """aog_step_pipelined against aog_step at o = 16: every output of every step bit for bit, two episodes."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A, N, T = 70, 16, 64, 5
    kw = dict(atm_type=atm, atm_vel=20.0 if atm == "dynamic" else 0, act_dim=A, obs_dim=16, rew_type="smf_ssim", num_pupil_pixels=N,
              timesteps_per_episode=T, seed=9, screen_oversampling=4, verbose=False)
    acts = torch.from_numpy(np.random.RandomState(3).randn(2 * T, B, A).astype(np.float32)).cuda()

    def run(pipelined):
        env = BatchedAOEnv(B, "cuda:0", **kw)
        assert _separable(env)
        outs = []
        for ep in range(2):
            obs0, _ = env.reset()
            outs.append(obs0.clone())
            for t in range(T):
                k = ep * T + t
                r = env.step(acts[k], next_actions=acts[k + 1] if t + 1 < T else None) if pipelined else env.step(acts[k])
                outs.extend([r[0].clone(), r[1].clone(), r[2].clone(), r[4]["obs_raw"].clone(), r[4]["power"].clone()])
        env.close()
        return outs

    plain, piped = run(False), run(True)
    assert len(plain) == len(piped)
    for a, b in zip(plain, piped):
        assert torch.equal(a, b)


def test_lookahead_bit_identical_dynamic_o8():
    """Lookahead on (the extrusion of step t + 1 launched behind this step's last screen reader) against off, dynamic o = 8."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A, N, T = 40, 16, 96, 6
    kw = dict(atm_type="dynamic", atm_vel=15.0, act_dim=A, obs_dim=8, num_pupil_pixels=N, timesteps_per_episode=T, seed=4,
              screen_oversampling=4, verbose=False)
    acts = torch.from_numpy(np.random.RandomState(8).randn(T, B, A).astype(np.float32)).cuda()

    def run(look):
        env = BatchedAOEnv(B, "cuda:0", **kw)
        assert _separable(env)
        env.lookahead(look)
        env.reset()
        outs = []
        for t in range(T):
            r = env.step(acts[t])
            outs.extend([r[0].clone(), r[1].clone(), r[4]["obs_raw"].clone(), r[4]["power"].clone()])
        assert env.device_status() == 0
        env.close()
        return outs

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_state_restore_reproduces_observations(precision):
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A, N = 12, 16, 64
    env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=10.0, act_dim=A, obs_dim=12, num_pupil_pixels=N, timesteps_per_episode=20,
                       seed=6, screen_oversampling=4, precision=precision, verbose=False)
    assert _separable(env)
    env.reset()
    gen = torch.Generator("cuda").manual_seed(2)
    acts = [torch.randn((B, A), device="cuda", generator=gen) for _ in range(6)]
    for a in acts[:2]:
        env.step(a)
    st = env.get_state()
    first = [env.step(a)[4]["obs_raw"].clone() for a in acts[2:]]
    env.set_state(st)
    again = [env.step(a)[4]["obs_raw"].clone() for a in acts[2:]]
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    env.close()


def test_shack_hartmann_o8_against_oracle():
    """SH_step then step at o = 8: the oracle's photon-noisy image replayed into the estimator, the step's observation and SSIM reward."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from oracle.ao_env_oracle import AOEnvOracle

    B, N, A, o = 3, 96, 20, 8
    kw = dict(atm_type="quasi_static", act_type="zernike", act_dim=A, obs_dim=o, rew_type="smf_ssim", timesteps_per_episode=5,
              SH_operation=True)
    scr = smooth_screens(B, N, 17)
    env = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, screens=scr, sh_fft_precision="double", verbose=False, **kw)
    assert _separable(env)
    refs = [AOEnvOracle(num_pupil_pixels=N, screen=scr[b].ravel(), rng=np.random.RandomState(40 + b), verbose=False, **kw) for b in range(B)]
    env.reset()
    for b in range(B):
        refs[b].reset()
        _obs_close(env.last_obs_raw[b].double().cpu().numpy(), refs[b].last_obs_raw)
    for t in range(2):
        img = env.sh_image()
        r_act = []
        for b in range(B):
            r_act.append(refs[b].SH_step()[0])
            img[b] = torch.from_numpy(np.round(refs[b].last_sh_noisy)).to(img.device)
        a = env.sh_update(img)
        _, rew, done, _, info = env.step(a)
        for b in range(B):
            _, r_rew, r_done, _, r_info = refs[b].step(r_act[b])
            _obs_close(info["obs_raw"][b].double().cpu().numpy(), refs[b].last_obs_raw)
            np.testing.assert_allclose(float(info["power"][b]), r_info["power"], rtol=RTOL)
            np.testing.assert_allclose(float(rew[b]), r_rew, rtol=RTOL, atol=1e-7)
            assert bool(done[b]) == r_done
    env.close()


@pytest.mark.parametrize("o", [16, 32])
def test_rollout_takes_the_hip_actor(o):
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.rollout import make_actor, rollout

    B, A, T = 8, 64, 4
    env = BatchedAOEnv(B, "cuda:0", act_dim=A, obs_dim=o, num_pupil_pixels=64, timesteps_per_episode=T, screens=smooth_screens(B, 64, 1),
                       verbose=False)
    out = rollout(env, make_actor(o * o, A, 64, device="cuda:0"), episodes=1, actor_impl="hip")
    assert out["obs"].shape == (T, B, o * o) and out["obs"].dtype == torch.float16
    assert bool(torch.isfinite(out["rew"]).all()) and bool(out["done"][T - 1].all())
    assert float(out["obs"].float().sum()) > 0
    env.close()


def test_gym_make_obs_dim16_episode_against_oracle():
    """gym.make('AO-v0', obs_dim=16) through the reference's entry path (child process: the gymnasium stand-in goes on sys.path first),
    one full episode against the oracle on the same screen."""
    script = textwrap.dedent('''
        import sys
        sys.path[:0] = [{root!r}, {fake!r}, {tests!r}]
        import numpy as np
        import gymnasium as gym
        import gym_AO
        from helpers import smooth_screens
        from oracle.ao_env_oracle import AOEnvOracle
        N, T, o = 64, 4, 16
        scr = smooth_screens(1, N, 5)
        kw = dict(atm_type="quasi_static", act_type="num_actuators", act_dim=16, obs_dim=o, rew_type="strehl_ratio", timesteps_per_episode=T)
        env = gym.make("AO-v0", num_pupil_pixels=N, screens=scr, verbose=False, **kw)
        assert env.observation_space.shape == (o * o,)
        ref = AOEnvOracle(num_pupil_pixels=N, screen=scr[0].ravel(), verbose=False, **kw)
        obs, _ = env.reset()
        ref.reset()
        rng = np.random.RandomState(0)
        for t in range(T):
            a = rng.randn(16).astype(np.float32)
            obs, rew, done, trunc, info = env.step(a)
            r_obs, r_rew, r_done, _, r_info = ref.step(a)
            assert obs.shape == (o * o,) and obs.dtype == np.float16
            got, want = np.asarray(obs, dtype=np.float64), np.asarray(r_obs, dtype=np.float64)
            ulp = np.abs(np.asarray(obs, np.float16).view(np.int16).astype(int) - np.asarray(r_obs, np.float16).view(np.int16).astype(int))
            assert ulp.max() <= 1, ulp.max()
            assert abs(rew - r_rew) <= 1e-3 and done == r_done
            assert abs(info["power"] - r_info["power"]) <= 1e-5 * abs(r_info["power"])
        assert done
        print("gym.make obs_dim=16 ok")
    ''').format(root=ROOT, fake=os.path.join(ROOT, "tests", "fake_gymnasium"), tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gym.make obs_dim=16 ok" in r.stdout


@pytest.mark.parametrize("precision,o", [("fast", 2), ("fast", 5), ("fp64", 5), ("fp64", 7)])
def test_sizes_below_the_new_route_keep_the_table_route(precision, o):
    _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    env = BatchedAOEnv(2, "cuda:0", act_dim=8, obs_dim=o, num_pupil_pixels=32, screens=smooth_screens(2, 32, 3), precision=precision,
                       verbose=False)
    assert not _separable(env) and env.obs_route == "tables"
    assert env.tables.wfs_coef.shape[0] == o * o + env.tables.n_fiber_modes
    env.close()


def test_separable_handle_refuses_to_step_before_the_matrices():
    """A separable handle whose aog_upload_obs_mft has not been made: aog_reset and aog_step return AOG_ERR_STATE."""
    torch = _torch()
    from adaptive_optics_gym_amd import _lib
    from adaptive_optics_gym_amd.optics_host import build_tables
    from adaptive_optics_gym_amd.params import OpticalParams

    lib = _lib.load()
    N, A, o, B = 32, 8, 12, 2
    t = build_tables(OpticalParams(num_pupil_pixels=N), "zernike", A, o, obs_route="separable")
    cfg = _lib.AogConfig()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.num_envs, cfg.n_pupil, cfg.n_modes, cfg.obs_dim, cfg.n_ap = B, N, A, o, t.n_ap
    cfg.n_wfs_tables, cfg.n_sci_tables, cfg.n_fiber_modes = t.wfs_tables.shape[0], t.sci_tables.shape[0], t.n_fiber_modes
    cfg.max_steps, cfg.obs_separable = 4, 1
    cfg.wavelength_wfs, cfg.wavelength_sci, cfg.surface_rms_target, cfg.ssim_ref_peak, cfg.ssim_alpha = 1.5e-6, 2.2e-6, 2.2e-7, 2.8, 0.8
    h = ctypes.c_void_p()
    _lib.check(lib.aog_create(ctypes.byref(cfg), 0, ctypes.byref(h)))
    keep = [np.ascontiguousarray(x) for x in (t.ap_index.astype(np.int32), t.modes, t.gram, t.wfs_tables, t.sci_tables,
                                               np.stack([t.wfs_coef.real, t.wfs_coef.imag], -1), np.stack([t.sci_coef.real, t.sci_coef.imag], -1))]
    P = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))  # noqa: E731
    tabs = _lib.AogTables(P(keep[0], ctypes.c_int32), *[P(k, ctypes.c_double) for k in keep[1:]], None, None, 0)
    _lib.check(lib.aog_upload_tables(h, ctypes.byref(tabs)))
    scr = torch.zeros((B, N, N), dtype=torch.float64, device="cuda")
    _lib.check(lib.aog_set_screens_f64(h, ctypes.c_void_p(scr.data_ptr()), 0, B, None))
    assert lib.aog_reset(h, None, None, None, None) == -3
    assert b"aog_upload_obs_mft" in lib.aog_last_error()
    act = torch.zeros((B, A), dtype=torch.float32, device="cuda")
    outs = [torch.zeros(B, device="cuda") for _ in range(3)]
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rc = lib.aog_step(h, ctypes.c_void_p(act.data_ptr()), None, None, ctypes.c_void_p(outs[0].data_ptr()), ctypes.c_void_p(done.data_ptr()),
                      ctypes.c_void_p(outs[1].data_ptr()), None, None)
    assert rc == -3
    torch.cuda.synchronize()
    lib.aog_destroy(h)
