"""The modulated pyramid wavefront sensor on the device (aog_upload_pyramid / aog_pyramid_frames / aog_pyramid_slopes / aog_pyramid_update)
against the float64 restatement of the model in pyramid_reference.py: frames and slopes over the launch geometries, independence of how
envs are grouped, the photon stream, the integrator loop, the layered atmosphere and the refusals."""
import numpy as np
import pytest

import pyramid_reference as ref
from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

# Worst |frame - reference| / (reference frame's peak) measured over MATRIX (the issue's whole cross product and its N = 96 case, both
# precisions) on an MI355X (profiles/pyramid_wfs.md), and the bounds held: 4 x.
FP64_WORST, FAST_WORST = 3.7e-15, 5.9e-7
FP64_BOUND, FAST_BOUND = 4 * FP64_WORST, 4 * FAST_WORST
# The slopes are differences of four pixels over the mean quadrant sum Ibar: a frame error eps x peak moves a slope by at most
# (4 + 4 |s|) eps x peak / Ibar — the slope bound follows from the frame bound, nothing else is measured for it.  The factor held is the one
# of |s| <= 1; a pixel brighter than the mean (|s| up to ~4 unmodulated) is held to it all the same, which asks more than the propagation.
SLOPE_FACTOR = 8.0

# (N, B, act_type, A, w_q, n_s, n_mod, r_mod).  MATRIX: B 3 / 33 (an env tile crossed, pad envs) x 6 Zernike / 20 actuators x w = 32 (one block) /
# 64 (shared form) / 96 (a third block) x n_s 16 / 24 x unmodulated / 8 points, and N = 96 (Nxp != N) with n_s = 40 (two detector blocks).
# EDGES, held to the same bounds: windows that are no multiple of 32 and quadrants that are no multiple of 16 (w = 48: the two halves share
# a k-step and a block's tail is empty; w = 80: an empty tail in the third block) with an n_s that divides nothing.
MATRIX = [(64, B, t, A, wq, ns, nm, rm) for B in (3, 33) for t, A in (("zernike", 6), ("num_actuators", 20)) for wq in (16, 32, 48) for ns in (16, 24)
          for nm, rm in ((1, 0.0), (8, 3.0))] + [(96, 3, "num_actuators", 20, 32, 40, 8, 3.0)]
EDGES = [(64, 3, "zernike", 6, 24, 16, 8, 3.0), (64, 33, "num_actuators", 20, 40, 20, 1, 0.0)]
CASES = MATRIX + EDGES
IDS = ["N%d-B%d-%s%d-wq%d-ns%d-mod%d" % c[:7] for c in CASES]
KW = dict(obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=5, verbose=False)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _sensor_kw(c):
    return dict(samples=c[4], pixels=c[5], n_mod=c[6], r_mod=c[7])


_RUNS = {}


def _run(case, precision):
    """reset, one step, frames and slopes on the device; the reference's frames and slopes of the sampled envs.  Once per (case, precision)."""
    key = (case, precision)
    if key in _RUNS:
        return _RUNS[key]
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    N, B, act_type, A = case[:4]
    scr = smooth_screens(B, N, 70 + N, amp=1e-5)
    a = actions_for(B, A, 4)
    env = BatchedAOEnv(B, "cuda:0", act_type=act_type, act_dim=A, num_pupil_pixels=N, screens=scr, precision=precision, pyramid=_sensor_kw(case), **KW)
    env.reset()
    env.step(torch.from_numpy(a).cuda())
    frames = env.pyramid_frames().cpu().numpy()
    slopes = env.pyramid_slopes().cpu().numpy()
    act = env.get_actuators().cpu().numpy()
    sensor = ref.Sensor(N, env.tables.ap_index, **_sensor_kw(case))
    want = {}
    for b in sorted({0, B // 2, B - 1}):
        f = sensor.frame(ref.phase_rev(scr[b], env.tables.modes, act[b], env.tables.ap_index, env.wavelength_wfs))
        want[b] = (f, sensor.slopes_of(f))
    assert np.array_equal(np.asarray(env._pyramid.valid), sensor.valid)
    env.close()
    _RUNS[key] = frames, slopes, want, sensor
    return _RUNS[key]


def _check(case, precision, bound):
    frames, slopes, want, sensor = _run(case, precision)
    N, B = case[:2]
    ns = case[5]
    assert frames.shape == (B, 4, ns, ns) and frames.dtype == np.float64 and slopes.shape == (B, 2 * sensor.valid.size)
    worst = worst_s = 0.0
    for b, (f, s) in want.items():
        worst = max(worst, float(np.abs(frames[b] - f).max() / f.max()))
        ibar = f.reshape(4, -1)[:, sensor.valid].sum(0).mean()
        worst_s = max(worst_s, float(np.abs(slopes[b] - s).max() / (SLOPE_FACTOR * f.max() / ibar)))
    print(f"pyramid {precision} {case}: worst frame error {worst:.3e} of the peak, worst slope error {worst_s:.3e} in the same units")
    assert worst <= bound, f"frames: {worst:.3e} > {bound:.3e}"
    assert worst_s <= bound, f"slopes: {worst_s:.3e} > {bound:.3e}"
    # a slope is a signed sum of the pixel's four values over Ibar: never beyond the pixel's own total over Ibar
    tot = frames.reshape(B, 4, -1)[:, :, sensor.valid].sum(axis=1)
    cap = np.tile(tot / tot.mean(axis=1, keepdims=True), (1, 2)) * (1 + 1e-12)
    assert float(frames.min()) >= 0 and bool((np.abs(slopes) <= cap).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frames_and_slopes_match_the_reference_fast(case):
    _check(case, "fast", FAST_BOUND)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frames_and_slopes_match_the_reference_fp64(case):
    _check(case, "fp64", FP64_BOUND)


def test_valu_kernel_handles_are_served():
    """The sensor reads psi_tile and operands of its own, so a handle that steps with the VALU kernel gets the same frames bit for bit."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A = 5, 64, 20
    scr, a = smooth_screens(B, N, 3, amp=1e-5), torch.from_numpy(actions_for(B, A, 2)).cuda()
    out = []
    for kernel in ("mfma", "valu"):
        env = BatchedAOEnv(B, "cuda:0", act_dim=A, num_pupil_pixels=N, screens=scr, kernel=kernel, pyramid=dict(samples=16, pixels=16), **KW)
        env.reset()
        env.step(a)
        out.append(env.pyramid_frames().clone())
        env.close()
    assert torch.equal(out[0], out[1]) and float(out[0].max()) > 0


def test_grouping_masks_and_chunks_change_no_bit(monkeypatch):
    """Two handles of 35 with their env_id_base equal one of 70 (photon noise on: the stream is keyed by the global env id), a mask leaves
    the other rows untouched, and chunks of 32 envs give the plain run's bits."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A = 70, 64, 20
    scr = smooth_screens(B, N, 21, amp=1e-5)
    a = torch.from_numpy(actions_for(B, A, 8)).cuda()
    sensor = dict(samples=32, pixels=24, n_mod=3, r_mod=2.0, photons=50.0)

    def run(n, offset, chunk=None, mask=None):
        if chunk:
            monkeypatch.setenv("AOG_PYRAMID_CHUNK", str(chunk))
        else:
            monkeypatch.delenv("AOG_PYRAMID_CHUNK", raising=False)
        env = BatchedAOEnv(n, "cuda:0", act_dim=A, num_pupil_pixels=N, screens=scr[offset:offset + n], global_env_offset=offset, total_envs=B, seed=11,
                           pyramid=sensor, **KW)
        env.reset()
        env.step(a[offset:offset + n])
        if mask is None:
            f = env.pyramid_frames()
        else:
            f = torch.full((n, 4, 24, 24), -7.0, dtype=torch.float64, device="cuda:0")
            env.pyramid_frames(mask=mask, out=f)
        env.close()
        return f.clone()

    plain = run(B, 0)
    assert torch.equal(torch.cat([run(35, 0), run(35, 35)]), plain)
    assert torch.equal(run(B, 0, chunk=32), plain)
    m = np.arange(B) % 3 == 0
    got = run(B, 0, mask=m)
    sel = torch.from_numpy(m).cuda()
    assert torch.equal(got[sel], plain[sel]) and bool((got[~sel] == -7.0).all())


def _blob(torch, env):
    """The library's state blob in a zeroed buffer (its parts start on 256-byte boundaries: the gaps between them are never written)."""
    import ctypes as C

    blob = torch.zeros((int(env.lib.aog_state_bytes(env._handle)),), dtype=torch.uint8, device="cuda:0")
    ts = C.c_int64()
    rc = env.lib.aog_get_state(env._handle, C.c_void_p(blob.data_ptr()), C.byref(ts), env._stream())
    assert rc == 0, env.lib.aog_last_error()
    torch.cuda.synchronize()
    return blob, int(ts.value)


@pytest.mark.parametrize("atm, kernel", [("quasi_static", "auto"), ("dynamic", "auto"), ("dynamic", "valu")])
def test_the_step_path_is_untouched(atm, kernel):
    """aog_step outputs, screens, actuators and the state blob of a handle, bit for bit, whether or not the sensor was called between steps.
    The dynamic VALU handle is the one whose psi_tile a sensor call rewrites and puts back: the blob carries it."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, T, A = 40, 4, 16
    kw = dict(atm_type=atm, atm_vel=20.0 if atm == "dynamic" else 0, atm_fried=0.15, act_dim=A, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=64,
              timesteps_per_episode=T, seed=9, screen_oversampling=4, kernel=kernel, verbose=False)
    acts = torch.from_numpy(np.random.RandomState(5).randn(T, B, A).astype(np.float32)).cuda()
    env, twin = BatchedAOEnv(B, "cuda:0", pyramid=dict(samples=16, pixels=16, n_mod=4, r_mod=2.0), **kw), BatchedAOEnv(B, "cuda:0", **kw)
    try:
        assert torch.equal(env.reset()[0], twin.reset()[0])
        env.pyramid_frames()
        for t in range(T):
            r1, r2 = env.step(acts[t]), twin.step(acts[t])
            s = env.pyramid_slopes()   # between every two steps of the episode
            assert bool(torch.isfinite(s).all())
            for k, name in ((0, "obs"), (1, "reward"), (2, "done")):
                assert torch.equal(r1[k], r2[k]), f"step {t}: {name} moved"
            for k in ("power", "strehl", "obs_raw"):
                assert torch.equal(r1[4][k], r2[4][k]), f"step {t}: {k} moved"
            assert torch.equal(env.get_actuators(), twin.get_actuators()), f"step {t}: the mirror moved"
        assert torch.equal(env.get_screens(), twin.get_screens())
        (b1, t1), (b2, t2) = _blob(torch, env), _blob(torch, twin)
        # the blob's 256-byte tail carries the sensor's own frame count (bytes 32 .. 40: after timestep, rng_seed, sh_calls, steps_since_reset
        # and obs_frame); every other byte is the twin's
        frame = lambda b: int(b[-256 + 32:-256 + 40].cpu().numpy().view(np.uint64)[0])
        assert frame(b1) == env.pyramid_frame_count == T + 1 and frame(b2) == 0
        b1[-256 + 32:-256 + 40] = 0
        assert t1 == t2 and b1.numel() > 0 and torch.equal(b1, b2), "the state blob moved"
        assert env.device_status() == 0
    finally:
        env.close()
        twin.close()


def test_photon_noise_follows_the_reference_stream():
    """Draws equal the host replay of the stream, the frame counter advances by one per sensor call of any kind, means are right, and
    photons=None reproduces the clean frame bit for bit whatever the counter says (no random word is drawn)."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A, seed, base = 6, 64, 6, 77, 100
    scr = smooth_screens(B, N, 9, amp=1e-5)
    cfg = dict(samples=16, pixels=16, n_mod=2, r_mod=1.0)
    mk = lambda photons: BatchedAOEnv(B, "cuda:0", act_type="zernike", act_dim=A, num_pupil_pixels=N, screens=scr, seed=seed, global_env_offset=base,
                                      total_envs=base + B, pyramid=dict(cfg, photons=photons), **KW)
    clean_env = mk(None)
    clean_env.reset()
    clean = clean_env.pyramid_frames().cpu().numpy()
    assert np.array_equal(clean_env.pyramid_frames().cpu().numpy(), clean) and clean_env.pyramid_frame_count == 2
    clean_env.close()
    sensor = ref.Sensor(N, clean_env.tables.ap_index, **cfg)
    for photons in (3.0, 400.0):   # (both branches of the sampler: counts below and above 12)
        env = mk(photons)
        env.reset()
        for call in range(3):
            got = (env.pyramid_frames() if call != 1 else None)
            if call == 1:
                env.pyramid_slopes()   # (counts as a frame)
                continue
            want, und = sensor.noisy(clean, photons, base + np.arange(B), env._base_seed, call)
            g = got.cpu().numpy()
            assert und.mean() < 1e-3
            np.testing.assert_array_equal(g[~und], want[~und])
            assert abs(g.mean() / clean.mean() - 1) < 5 / np.sqrt(photons * clean.sum())   # (5 sigma of the total count)
        assert env.pyramid_frame_count == 3
        env.close()


def test_the_integrator_follows_the_reference_loop():
    """PYR_step over 10 iterations on a quasi-static env (N = 64, 20 modes) against the reference loop run with the env's own command matrix
    on the same screens: every actuator within ||R|| x the slope bound x the gain, accumulated over the steps so far; the device
    calibration against the reference's; rollout(policy='pyramid') runs with rollout's shapes and log_prob 1."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.rollout import rollout

    B, N, A, T = 3, 64, 20, 10
    scr = smooth_screens(B, N, 31, amp=4e-6)
    cfg = dict(samples=16, pixels=16, n_mod=12, r_mod=1.5, gain=0.4)
    env = BatchedAOEnv(B, "cuda:0", act_dim=A, num_pupil_pixels=N, screens=scr, SH_operation=True, pyramid=cfg, **dict(KW, timesteps_per_episode=T))
    sensor = ref.Sensor(N, env.tables.ap_index, **{k: cfg[k] for k in ("samples", "pixels", "n_mod", "r_mod")})
    modes, lam = env.tables.modes, env.wavelength_wfs
    env.reset()
    got = []
    for _ in range(T):
        act, slopes = env.PYR_step()
        got.append(act.cpu().numpy())
        env.step(act)
    R, s_ref = env.pyramid_reconstructor, env.pyramid_reference_slopes
    # the calibration itself: response and reference slopes against the reference's, in units of the slope bound
    R_ref, s_ref_ref, resp_ref = ref.calibrate(sensor, modes, lam, env.pyramid["poke"], env.pyramid["rcond"])
    flat = sensor.frame(np.zeros(sensor.n_ap))
    unit = SLOPE_FACTOR * FAST_BOUND * flat.max() / flat.reshape(4, -1)[:, sensor.valid].sum(0).mean()
    assert np.abs(s_ref - s_ref_ref).max() <= unit
    assert np.abs(env.pyramid_response - resp_ref).max() <= 2 * unit / (2 * env.pyramid["poke"])
    norm_R = np.abs(R).sum(axis=1).max()   # (the infinity norm: a slope error of `unit` per entry moves an actuator by at most this x unit)
    worst = 0.0
    for b in range(B):
        want, _ = ref.integrate(sensor, scr[b], modes, lam, R, s_ref, cfg["gain"], T)
        rms = [ref.residual_rms(scr[b], modes, a, env.tables.ap_index, lam) for a in want]
        assert rms[-1] < rms[0]
        for t in range(T):
            err = np.abs(got[t][b] - want[t + 1]).max() / (norm_R * unit * cfg["gain"] * (t + 1) * 2)
            worst = max(worst, float(err))
    print(f"pyramid integrator: worst actuator error {worst:.3f} of ||R|| x bound (accumulated)")
    assert worst <= 1.0
    torch.manual_seed(3)
    out = rollout(env, None, episodes=1, policy="pyramid")
    assert out["act"].shape == (T, B, A) and out["obs"].shape[:2] == (T, B) and bool((out["log_prob"] == 1).all())
    env.close()


def test_layered_env_slopes_equal_a_static_env_on_the_layer_sum():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    B, N, A = 4, 64, 16
    cfg = dict(samples=16, pixels=16, n_mod=4, r_mod=2.0)
    kw = dict(act_dim=A, num_pupil_pixels=N, **KW)
    lay = LayeredAOEnv(B, "cuda:0", atm_layers=[dict(fraction=0.6, speed=10.0), dict(fraction=0.4, speed=25.0)], seed=5, screen_oversampling=4, pyramid=cfg, **kw)
    lay.reset()
    a = torch.from_numpy(actions_for(B, A, 1)).cuda()
    lay.step(a)
    got = lay.pyramid_slopes().clone()
    static = BatchedAOEnv(B, "cuda:0", screens=lay.get_screens().cpu().numpy(), pyramid=cfg, **kw)
    static.reset()
    static.set_actuators(lay.get_actuators())
    want = static.pyramid_slopes()
    torch.testing.assert_close(got, want, rtol=0, atol=SLOPE_FACTOR * FAST_BOUND * 4)
    lay.close()
    static.close()


def test_refusals():
    torch = _torch()
    import ctypes as C

    from adaptive_optics_gym_amd import BatchedAOEnv, _lib

    B, N, A = 5, 64, 16
    kw = dict(act_dim=A, num_pupil_pixels=N, screens=smooth_screens(B, N, 2), **KW)
    for bad in (dict(samples=7), dict(samples=65), dict(pixels=7), dict(pixels=65), dict(n_mod=0), dict(n_mod=33), dict(r_mod=-1.0),
                dict(samples=8, r_mod=3.5), dict(photons=-1.0), dict(colour=1)):
        with pytest.raises(ValueError, match="pyramid"):
            BatchedAOEnv(B, "cuda:0", pyramid=bad, **kw)
    plain = BatchedAOEnv(B, "cuda:0", **kw)
    base = plain.device_bytes()
    for call in (plain.pyramid_frames, plain.pyramid_slopes, plain.PYR_step, plain.pyramid_calibrate):
        with pytest.raises(ValueError, match="pyramid sensor"):
            call()
    buf = torch.zeros(B * 4 * 64 * 64, dtype=torch.float64, device="cuda:0")
    assert plain.lib.aog_pyramid_frames(plain._handle, None, C.c_void_p(buf.data_ptr()), None) == -3 and b"not uploaded" in plain.lib.aog_last_error()
    assert plain.lib.aog_pyramid_update(plain._handle, 0.4, C.c_void_p(buf.data_ptr()), None, None) == -3
    assert plain.lib.aog_upload_pyramid_reconstructor(plain._handle, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr())) == -3
    t = _lib.AogPyramidTables(4, 16, 1, 1, *([None] * 9), 1.0, 1.0, 0.0)
    assert plain.lib.aog_upload_pyramid(plain._handle, C.byref(t)) == -1 and b"samples" in plain.lib.aog_last_error()
    assert plain.device_bytes() == base
    plain.close()
    env = BatchedAOEnv(B, "cuda:0", pyramid=dict(samples=16, pixels=16), **kw)
    assert env.device_bytes() > base
    env.reset()
    assert env.lib.aog_pyramid_update(env._handle, 0.4, C.c_void_p(buf.data_ptr()), None, None) == -3 and b"reconstructor" in env.lib.aog_last_error()
    acts = torch.from_numpy(np.random.RandomState(6).randn(2, B, A).astype(np.float32)).cuda()
    env.step(acts[0], next_actions=acts[1])   # mid-sequence: the mirror already belongs to the next step
    for call in (env.pyramid_frames, env.pyramid_slopes):
        with pytest.raises(_lib.AogError, match="libaogym error -3"):
            call()
    env.step(acts[1], next_actions=None)
    assert float(env.pyramid_frames().max()) > 0
    with pytest.raises(ValueError, match="mask"):
        env.pyramid_frames(mask=np.ones(B + 1, dtype=bool))
    env.close()
