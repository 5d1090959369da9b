"""Every entry point that takes a stream, run on a caller's side stream behind a delayed producer (``stream_harness``) and held bit for bit
to a twin handle that makes the same calls on the default stream.  The twin is the reference here: the oracle tests hold the default stream.

Exceptions, the project's stated ones and only those: results downstream of ``k_sh_estimate`` (float64 LDS atomics, equal to rounding:
``rtol=1e-10`` as in ``test_gpu_parity.test_shack_hartmann_chain_matches_oracle``) and the policy query's ``log_prob`` (float atomics in an
unfixed order: ``1e-6`` as in ``test_gpu_step_act`` / ``test_gpu_rollout_policies.test_actor_hip_query``).

The delay of a producer is max(``FLOOR_MS`` x the library calls behind it, 10 x the host-side duration of those calls, measured on the twin
just before); ``torch.cuda._sleep`` is calibrated once per module with two events.  Each test prints its delays, that duration and the
tightest self-check: how much host time had passed behind a producer when a call returned, against that producer's delay (``-s``).

Host values (``set_turbulence``'s Fried parameters, ``set_detector``'s photon numbers) cannot be produced on the device behind the delay:
those calls are made behind the delay, directly in front of the reset / step that reads what they copy on the stream.
"""
import time

import numpy as np
import pytest

import stream_harness as sh
from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

SH_RTOL = 1e-10       # test_gpu_parity.test_shack_hartmann_chain_matches_oracle: the estimator's float64 LDS atomics
LOGP_RTOL = 1e-6      # test_gpu_step_act / test_gpu_rollout_policies.test_actor_hip_query: aog_actor_act's float atomics

# entry point (include/aogym.h, every one with a `void* stream`) -> the test here that drives it through Python
COVERED = {
    "aog_set_screens_f64": "test_state_and_screens", "aog_set_screens_f32": "test_state_and_screens",
    "aog_set_wind": "test_dynamic",   # (constructor only: made with the side stream current and synchronised there, never behind the delay)
    "aog_set_extrusion_noise": "test_dynamic", "aog_evolve_atmosphere": "test_dynamic",
    "aog_get_screens_f64": "test_dynamic", "aog_install_layer_sum": "test_layered",
    "aog_generate_screens": "test_device_screens", "aog_get_phase_screen": "test_device_screens",
    "aog_set_turbulence": "test_per_env_turbulence", "aog_set_detector": "test_detector",
    "aog_sh_image": "test_shack_hartmann", "aog_sh_update": "test_shack_hartmann",
    "aog_get_state": "test_state_and_screens", "aog_set_state": "test_state_and_screens",
    "aog_get_actuators": "test_state_and_screens", "aog_set_actuators": "test_state_and_screens",
    "aog_reset": "test_step_table_route", "aog_step": "test_step_table_route", "aog_step_pipelined": "test_step_table_route",
    "aog_focal_image": "test_instruments_first_call", "aog_focal_images": "test_instruments_first_call",
    "aog_wavefront_truth": "test_instruments_first_call", "aog_output_gradient": "test_instruments_first_call",
    "aog_science_integrate": "test_instruments_first_call", "aog_science_clear": "test_instruments_first_call",
    "aog_science_read": "test_instruments_first_call",
    "aog_pyramid_frames": "test_instruments_first_call", "aog_pyramid_slopes": "test_instruments_first_call",
    "aog_pyramid_update": "test_instruments_first_call", "aog_pyramid_gradient": "test_instruments_first_call",
    "aog_actor_act": "test_fused_policies", "aog_actor_act_noise": "test_fused_policies",
    "aog_reset_act": "test_fused_policies", "aog_step_act": "test_fused_policies",
    "aog_reset_act_noise": "test_fused_policies", "aog_step_act_noise": "test_fused_policies",
    "aog_reset_spgd": "test_fused_spgd", "aog_step_spgd": "test_fused_spgd",
    "aog_predictor_reset": "test_predictor", "aog_predictor_update": "test_predictor",
    "aog_predictor_get_state": "test_predictor", "aog_predictor_set_state": "test_predictor",
    "aog_telemetry_reset": "test_telemetry", "aog_telemetry_push": "test_telemetry", "aog_telemetry_psd": "test_telemetry",
    "aog_telemetry_gains": "test_telemetry", "aog_telemetry_get_state": "test_telemetry", "aog_telemetry_set_state": "test_telemetry",
    "aog_spgd_reset": "test_spgd_handle", "aog_spgd_update": "test_spgd_handle", "aog_spgd_get_state": "test_spgd_handle",
    "aog_spgd_set_state": "test_spgd_handle",
    "aog_link_reset": "test_link", "aog_link_push": "test_link", "aog_link_statistics": "test_link", "aog_link_get_state": "test_link",
    "aog_link_set_state": "test_link",
}
# (aog_reset_act / aog_step_act: the plain forms are the _noise forms with noise = NULL, which is what the wrappers call without OU noise)

# entry points with a stream that no public Python method calls, each with the reason it is not driven here
NOT_DRIVEN = {
    "aog_selftest_sincos": "selftest of a device function; tests call it through the raw library on the default stream",
    "aog_selftest_poisson": "selftest of a device function; tests call it through the raw library on the default stream",
    "aog_selftest_barrier_timeout": "developer aid: provokes the grid barrier's timeout path, not something to run beside other work",
}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cycles_per_ms():
    torch = _torch()
    c = sh.calibrate(torch)
    print(f"\n[streams] torch.cuda._sleep: {c:.0f} cycles per ms; hipStreamGetFlags of torch.cuda.Stream(): {sh.stream_flags(torch.cuda.Stream())}")
    return c


def _both(cycles_per_ms, make, script, rtol=None):
    """``script(handle, runner)`` on a default-stream twin, then on a like handle made and driven on a side stream; returns nothing,
    fails with every difference.  ``make()`` builds the handle (under test: inside the side stream's context, so that whatever the
    constructor allocates, zero-fills and uploads happens with that stream current)."""
    torch = _torch()
    twin_handle = make()
    twin = sh.Runner(torch)
    try:
        script(twin_handle, twin)
        longest, which = twin.longest()
        rejected = len(sh._REJECTED)
        side = sh.side_stream(torch, cycles_per_ms)
        rejected = len(sh._REJECTED) - rejected
        with torch.cuda.stream(side):
            handle = make()
        side.synchronize()
        run = sh.Runner(torch, side, cycles_per_ms, twin)
        try:
            script(handle, run)
            lines = sh.compare(torch, twin, run, rtol)
        finally:
            torch.cuda.synchronize()
            _close(handle)
    finally:
        torch.cuda.synchronize()
        _close(twin_handle)
    share, label, behind, delay = run.tightest
    print(f"\n[streams] delays {min(run.delays)[0]:.0f} .. {max(run.delays)[0]:.0f} ms; longest non-exempt chain behind one producer on the twin "
          f"{1e3 * longest:.3f} ms ({which}); tightest self-check: {behind:.2f} ms of host time behind a {delay:.0f} ms delay ({label}); "
          f"{len(run.outputs)} calls compared; {rejected} side streams turned down (they shared the null stream's queue)")
    assert not lines, "\n".join(lines)


def _close(h):
    for x in (h if isinstance(h, (tuple, list)) else (h,)):
        if hasattr(x, "close"):
            x.close()


def _env(B, N=64, **kw):
    from adaptive_optics_gym_amd import BatchedAOEnv

    base = dict(act_type="zernike", act_dim=6, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=50, num_pupil_pixels=N, verbose=False)
    base.update(kw)
    return BatchedAOEnv(B, "cuda:0", **base)


def _acts(B, A, seed, scale=1.0):
    return actions_for(B, A, seed) * np.float32(scale)


# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [("zernike", 6), ("num_actuators", 64)], ids=["zernike6", "act64"])
@pytest.mark.parametrize("precision,kernel", [("fast", "mfma"), ("fast", "valu"), ("fp64", "auto")])
def test_step_table_route(cycles_per_ms, precision, kernel, act):
    torch = _torch()
    B, N, (act_type, A) = 33, 64, act
    scr = smooth_screens(B, N, 3)
    mask = np.arange(B) % 3 == 1

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        for t in range(3):
            a = r.input(_acts(B, A, t))
            r.call(f"step{t}", lambda: env.step(a))
        m = r.input(mask)
        r.call("masked reset", lambda: env.reset(m)[0])
        out = (torch.zeros((B, 4), dtype=torch.float16, device="cuda"), torch.zeros((B,), device="cuda"), torch.zeros((B,), dtype=torch.bool, device="cuda"))
        a = r.input(_acts(B, A, 7))
        r.call("step(out=)", lambda: (env.step(a, out=out), out))
        env.persistent_outputs(True)
        a0, a1 = r.input(_acts(B, A, 8)), r.input(_acts(B, A, 9))
        r.call("persistent x2", lambda: [sh._clone(torch, env.step(a0)), env.step(a1)], weight=2)
        env.persistent_outputs(False)
        p0, p1, p2 = (r.input(_acts(B, A, 10 + i)) for i in range(3))
        r.call("pipelined x3", lambda: [env.step(p0, next_actions=p1), env.step(p1, next_actions=p2), env.step(p2, next_actions=None)], weight=3)
        r.call("device_status", lambda: env.device_status(), blocking="device_status")

    _both(cycles_per_ms, lambda: _env(B, N, act_type=act_type, act_dim=A, screens=scr, precision=precision, kernel=kernel), script)


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_separable_route(cycles_per_ms, precision):
    B, N, A = 5, 64, 6
    scr = smooth_screens(B, N, 4)

    def script(env, r):
        assert env.obs_route == "separable"
        r.call("reset", lambda: env.reset()[0])
        a = r.input(_acts(B, A, 1))
        r.call("step", lambda: env.step(a))

    _both(cycles_per_ms, lambda: _env(B, N, obs_dim=8, screens=scr, precision=precision), script)


@pytest.mark.parametrize("method", ["twoband", "hcipy16"])
@pytest.mark.parametrize("N", [64, 96])
def test_device_screens(cycles_per_ms, N, method):
    B = 3
    other = "hcipy16" if method == "twoband" else "twoband"

    def script(env, r):
        # (a fresh handle made on the side stream: the constructor's first synthesis allocated its workspace there)
        r.call("reset 1", lambda: (env.reset()[0], env.phase_screen(1)))
        r.call("reset 2", lambda: (env.reset()[0], env.phase_screen(2)))

        def switch():
            env.set_screen_method(other)
            return env.reset()[0], env.phase_screen(0)

        r.call("set_screen_method + reset", switch, blocking="screen_workspace")
        r.call("device_bytes", lambda: env.device_bytes(), blocking="device_bytes")

    _both(cycles_per_ms, lambda: _env(B, N, atm_type="semi_dynamic", seed=3, screen_method=method, screen_oversampling=4 if N == 96 else 16), script)


@pytest.mark.parametrize("lookahead", [False, True], ids=["plain", "lookahead"])
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
@pytest.mark.parametrize("N", [32, 64])
def test_dynamic(cycles_per_ms, N, extrusion, lookahead):
    torch = _torch()
    from adaptive_optics_gym_amd.atmosphere_host import integer_shifts

    B, A, T = 4, 6, 4

    def script(env, r):
        if lookahead:
            assert env.lookahead(True)
        r.call("reset", lambda: env.reset()[0])
        for t in range(T):
            a = r.input(_acts(B, A, t))
            # (the first step of a dynamic handle allocates and plans its work ahead: 6 .. 14 ms on the host behind a delayed stream)
            r.call(f"step{t}", lambda: env.step(a), weight=1 if t else 3)
        # (the episode has ended: with lookahead the screens are readable again only here)
        r.call("get_screens", lambda: env.get_screens())
        r.call("reset 2", lambda: env.reset()[0])
        if lookahead:
            env.lookahead(False)
        a = r.input(_acts(B, A, 9))
        r.call("step + evolve + get_screens", lambda: (env.step(a), env.evolve_atmosphere(), env.get_screens(1, 2)))
        state = r.call("get_state", lambda: env.get_state(), blocking="get_state")
        a = r.input(_acts(B, A, 10))
        r.call("step after get_state", lambda: env.step(a))
        if extrusion == "f64":
            shifts = integer_shifts(env.velocity_vectors, env.timestep * env.delta_t, (env.timestep + 1) * env.delta_t, env.params.pupil_pixel)
            rows = int(np.abs(shifts).sum(axis=1).max())
            if rows:
                n = r.input(np.random.RandomState(5).randn(B, rows, N))
                a = r.input(_acts(B, A, 11))
                r.call("set_extrusion_noise + step", lambda: (env.set_extrusion_noise(n), env.step(a))[1])
        blob = r.input(state["blob"])
        a = r.input(_acts(B, A, 12))
        r.call("set_state mid-episode + step", lambda: (env.set_state(dict(state, blob=blob)), env.step(a), env.get_screens())[1:], blocking="set_state")

    _both(cycles_per_ms, lambda: _env(B, N, atm_type="dynamic", atm_vel=20.0, seed=9, screen_oversampling=4, extrusion=extrusion, timesteps_per_episode=T), script)


@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_stream_change_mid_episode(cycles_per_ms, extrusion):
    """Step t on s1, s2.wait_stream(s1), step t + 1 on s2, then back on the default stream after a wait_stream, with no synchronisation in
    between: the handle's own event waits must follow the stream of the call, not that of the first call."""
    torch = _torch()
    B, A, N = 4, 6, 32

    def script(env, r):
        # (the further streams are drawn first: the probe that admits a side stream drains the device)
        s2, s3 = (sh.side_stream(torch, cycles_per_ms), sh.side_stream(torch, cycles_per_ms)) if r.side is not None else (None, None)
        for s in (s2, s3):   # (and each has made its first allocation: the caching allocator's first block of a stream is a hipMalloc)
            if s is not None:
                with torch.cuda.stream(s):
                    torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
                s.synchronize()
        r.call("reset", lambda: env.reset()[0])
        acts = [r.input(_acts(B, A, t)) for t in range(4)]
        r.call("step0 on s1", lambda: env.step(acts[0]), drain=False)
        r.use(s2)
        r.call("step1 on s2", lambda: env.step(acts[1]), lead=False, drain=False)
        r.use(s3)
        r.call("step2 on s3", lambda: env.step(acts[2]), lead=False, drain=False)
        r.use(torch.cuda.default_stream())
        r.call("step3 on the default stream", lambda: (env.step(acts[3]), env.get_screens()), lead=False, weight=2)

    _both(cycles_per_ms, lambda: _env(B, N, atm_type="dynamic", atm_vel=20.0, seed=9, screen_oversampling=4, extrusion=extrusion), script)


def test_layered(cycles_per_ms):
    from adaptive_optics_gym_amd import LayeredAOEnv

    B, A, N = 5, 6, 32
    layers = [{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}]

    def make():
        return LayeredAOEnv(B, "cuda:0", atm_layers=layers, atm_fried=0.15, seed=11, act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio",
                            timesteps_per_episode=5, num_pupil_pixels=N, verbose=False)

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        for t in range(3):
            a = r.input(_acts(B, A, t))
            r.call(f"step{t}", lambda: env.step(a), weight=len(layers) + 2)   # (every layer evolves, their sum is installed, then the step)
        r.call("get_screens", lambda: env.get_screens())

    _both(cycles_per_ms, make, script)


@pytest.mark.parametrize("o", [2, 8])
def test_detector(cycles_per_ms, o):
    B, A, N = 5, 6, 64
    scr = smooth_screens(B, N, 5)
    photons = np.linspace(2e3, 2e4, B)

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        a = r.input(_acts(B, A, 1))
        r.call("step", lambda: env.step(a))
        a = r.input(_acts(B, A, 2))
        r.call("set_detector + step", lambda: (env.set_detector(photons, read_noise=1.0), env.step(a))[1])
        a = r.input(_acts(B, A, 3))
        r.call("set_detector(None) + step + reset", lambda: (env.set_detector(None), env.step(a), env.reset()[0])[1:])

    _both(cycles_per_ms, lambda: _env(B, N, obs_dim=o, screens=scr, seed=5, obs_photons=1e4, obs_read_noise=2.0, obs_background=3.0), script)


def test_per_env_turbulence(cycles_per_ms):
    B, N = 3, 64
    fried = np.array([0.1, 0.15, 0.25])

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        r.call("set_turbulence + reset", lambda: (env.set_turbulence(fried), env.reset()[0], env.phase_screen(2))[1:])
        # (a host mask: a semi_dynamic reset reads its mask on the host to pick the envs whose screens it redraws)
        r.call("set_turbulence(mask) + masked reset", lambda: (env.set_turbulence(0.2, mask=[False, False, True]), env.reset([True, False, True])[0],
                                                               env.phase_screen(2))[1:], blocking="host_copy")

    _both(cycles_per_ms, lambda: _env(B, N, atm_type="semi_dynamic", seed=3), script)


@pytest.mark.parametrize("N,B,fft", [(128, 3, "single"), (96, 2, "single"), (96, 2, "double")])
def test_shack_hartmann(cycles_per_ms, N, B, fft):
    """Everything downstream of the estimator to SH_RTOL (float64 LDS atomics); the sensor image itself bit for bit."""
    A = 8
    scr = smooth_screens(B, N, 3) * 0.5
    noisy = np.round(np.random.RandomState(1).gamma(2.0, 50.0, size=(B, N * N)))

    def script(env, r):
        r.call("image: reset + sh_image", lambda: (env.reset()[0], env.sh_image()))
        n = r.input(noisy)
        r.call("sh_update(noisy)", lambda: env.sh_update(n), blocking="sh_update")
        r.call("SH_step x2", lambda: [env.SH_step()[0], env.SH_step()[0]], weight=4)
        act = r.call("SH_step", lambda: env.SH_step()[0])
        a = r.input(act.float())
        r.call("step", lambda: env.step(a))

    rtol = {k: SH_RTOL for k in ("sh_update(noisy)", "SH_step x2", "SH_step", "step")}   # (step: the action is the estimator's output)
    _both(cycles_per_ms, lambda: _env(B, N, act_dim=A, screens=scr, SH_operation=True, sh_fft_precision=fft), script, rtol=rtol)


@pytest.mark.parametrize("precision", ["fast", "fp64"])
@pytest.mark.parametrize("instrument", ["truth", "gradient", "obs_gradient", "science", "pyramid", "focal"])
def test_instruments_first_call(cycles_per_ms, instrument, precision):
    """A fresh handle per instrument: its first call, with the lazy zero-filled allocations and the upload of its tables, happens on the side
    stream; then the same calls again, warm."""
    torch = _torch()
    if instrument == "focal" and precision == "fp64":
        precision = "fast-valu"   # (focal_images is built for fast precision only: the second case runs the other fast kernel)
    B, A, N = 3, 6, 64
    o = 8 if instrument == "obs_gradient" else 2
    scr = smooth_screens(B, N, 6)
    kw = dict(obs_dim=o, screens=scr, precision="fast" if precision.startswith("fast") else "fp64", kernel="valu" if precision == "fast-valu" else "auto")
    if instrument == "obs_gradient":
        kw["obs_gradient"] = True
    if instrument == "science":
        kw["science_window"] = 16
    if instrument == "pyramid":
        kw["pyramid"] = dict(samples=16, pixels=16, n_mod=4, r_mod=2.0)
    rng = np.random.RandomState(2)
    g_obs, g_p, g_s, g_frames = rng.randn(B, o * o), rng.randn(B), rng.randn(B), rng.randn(B, 4, 16, 16)

    def calls(env, r, tag, first):
        # (the uploads of the wavefront fit and of the gradient's tables are blocking copies that wait for no stream: their first calls are
        # held to the self-check; a science camera's, a pyramid's and focal_images' first calls synchronise the device)
        up = "upload" if first and instrument in ("science", "pyramid", "focal") else None
        if instrument == "truth":
            r.call(f"{tag} wavefront_truth", lambda: env.wavefront_truth(), blocking=up)
            r.call(f"{tag} ideal_action", lambda: env.ideal_action())
        elif instrument in ("gradient", "obs_gradient"):
            go, gp, gs = r.input(g_obs), r.input(g_p), r.input(g_s)
            r.call(f"{tag} output_gradient(actuators)", lambda: env.output_gradient(go, gp, gs, with_values=True), blocking=up)
            go, gs = r.input(g_obs), r.input(g_s)
            r.call(f"{tag} output_gradient(action)", lambda: env.output_gradient(go, None, gs, wrt="action"))
        elif instrument == "science":
            m = np.array([True, False, True])   # (a mask goes to the device through a host copy, which waits for the stream)
            r.call(f"{tag} science", lambda: (env.science_integrate(), env.science_exposure(), env.science_clear(), env.science_integrate(),
                                              env.science_integrate(), env.science_exposure(1, 2, image=False)), blocking=up)
            r.call(f"{tag} science, masked", lambda: (env.science_integrate(m), env.science_exposure(), env.science_clear(m), env.science_exposure()),
                   blocking="host_copy")
        elif instrument == "pyramid":
            gf = r.input(g_frames)
            r.call(f"{tag} pyramid", lambda: (env.pyramid_frames(), env.pyramid_slopes(), env.pyramid_gradient(g_frames=gf, with_values=True)), blocking=up)
            r.call(f"{tag} PYR_step", lambda: env.PYR_step(), blocking="pyramid_calibrate" if first else None)
        else:
            r.call(f"{tag} focal_images in two chunks", lambda: (env.focal_images(0, 2), env.focal_images(2, 1), env.focal_image(1)), blocking=up)

    def script(env, r):
        a = r.input(_acts(B, A, 1))
        r.call("reset + step", lambda: (env.reset()[0], env.step(a)))
        calls(env, r, "first", True)
        a = r.input(_acts(B, A, 2))
        r.call("step", lambda: env.step(a))
        calls(env, r, "warm", False)

    _both(cycles_per_ms, lambda: _env(B, N, **kw), script)


def _named(x):
    """((step or reset result), (action, log_prob, mean) or None) with the policy's outputs under their names, for the log_prob tolerance."""
    res, pol = x
    return {"result": res, "policy": None if pol is None else {"action": pol[0], "log_prob": pol[1], "mean": pol[2]}}


def _actor(torch, A):
    from adaptive_optics_gym_amd.rollout import make_actor

    torch.manual_seed(5)
    actor = make_actor(4, A, 32, device="cuda:0")
    with torch.no_grad():
        actor.out.weight.mul_(100.0)
    return actor


def test_fused_policies(cycles_per_ms):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise, rollout

    B, A, N, T = 17, 6, 64, 3
    scr = smooth_screens(B, N, 8)
    actor = _actor(torch, A)

    def make():
        return _env(B, N, act_dim=A, screens=scr, timesteps_per_episode=T), DeviceActor(actor, seed=9), DeviceOUNoise(B, A, device="cuda:0")

    def script(h, r):
        env, da, ou = h
        r.call("reset_with_policy", lambda: _named(env.reset_with_policy(da)))
        r.call("step_with_policy x3", lambda: [sh._clone(torch, _named(env.step_with_policy(da))) for _ in range(T)], weight=T)
        r.call("eval with OU noise", lambda: [sh._clone(torch, _named(env.reset_with_policy(da, ou_noise=ou, action_mode="mean")))]
               + [sh._clone(torch, _named(env.step_with_policy(da, ou_noise=ou, action_mode="mean"))) for _ in range(T)] + [ou.state], weight=T + 1)
        obs = r.call("reset", lambda: env.reset()[0])
        o = r.input(obs)
        r.call("policy query", lambda: [_named((None, da(o))), _named((None, da(o, ou_noise=ou)))])
        r.call("rollout(actor, fused)", lambda: rollout(env, actor, episodes=2, actor_impl="hip", dev_actor=da, fused_policy=True), blocking="rollout")
        r.call("rollout(actor)", lambda: rollout(env, actor, episodes=1, actor_impl="hip", dev_actor=da), blocking="rollout")

    _both(cycles_per_ms, make, script, rtol={"log_prob": LOGP_RTOL})


@pytest.mark.parametrize("fused", [False, True])
def test_fused_spgd(cycles_per_ms, fused):
    torch = _torch()
    from adaptive_optics_gym_amd import LinkTelemetry
    from adaptive_optics_gym_amd.rollout import rollout
    from adaptive_optics_gym_amd.sensorless import SPGDController

    B, A, N, T = 17, 8, 64, 3
    scr = smooth_screens(B, N, 8) * 0.5

    def make():
        env = _env(B, N, act_dim=A, screens=scr, timesteps_per_episode=T, SH_operation=True, seed=5)
        return env, SPGDController(env, gain=2e-6, amplitude=np.linspace(2e-8, 4e-8, B), metric="strehl", seed=2024), LinkTelemetry(B, length=64, device="cuda:0")

    def script(h, r):
        env, ctrl, link = h
        r.call("reset_with_spgd", lambda: env.reset_with_spgd(ctrl))
        r.call("step_with_spgd x3", lambda: [sh._clone(torch, env.step_with_spgd(ctrl)) for _ in range(T)], weight=T)
        r.call("rollout(spgd, link=)", lambda: rollout(env, None, episodes=2, policy="spgd", controller=ctrl, fused_policy=fused, link=link), blocking="rollout")
        r.call("link.statistics", lambda: link.statistics(), blocking="host_copy")
        r.call("rollout(shack)", lambda: rollout(env, None, episodes=1, policy="shack"), blocking="rollout")
        r.call("spgd get_state", lambda: ctrl.get_state())

    _both(cycles_per_ms, make, script, rtol={"rollout(shack)": SH_RTOL})


# ----------------------------------------------------------------------------------------------------------------------------------------
# stand-alone handles
@pytest.mark.parametrize("A,p", [(16, 3), (40, 4)])
def test_predictor(cycles_per_ms, A, p):
    from adaptive_optics_gym_amd.predictor import DevicePredictor

    B = 3
    rows = np.random.RandomState(4).randn(6, B, A) * 1e-7

    def script(pred, r):
        for t in range(3):
            y = r.input(rows[t])
            r.call(f"update{t}", lambda: pred.update(y))
        y, m = r.input(rows[3]), r.input(np.array([True, False, True]))
        r.call("masked update", lambda: pred.update(y, mask=m))
        blob = r.call("get_state", lambda: pred.get_state())
        m = r.input(np.array([False, True, False]))
        y = r.input(rows[4])
        r.call("masked reset + update", lambda: (pred.reset(m), pred.update(y))[1])
        b = r.input(blob)
        y = r.input(rows[5])
        r.call("set_state + update", lambda: (pred.set_state(b), pred.update(y), pred.get_state())[1:], blocking="set_state")

    _both(cycles_per_ms, lambda: DevicePredictor(B, A, order=p, scale=1e-7, device="cuda:0"), script)


def test_telemetry(cycles_per_ms):
    from adaptive_optics_gym_amd import ModalTelemetry

    B, A, L = 3, 6, 64
    rows = np.random.RandomState(6).randn(L + 8, B, A)

    def script(tel, r):
        # (the handle is made by the first push: lazy.  18 rows per delay: every operation enqueued behind the delay costs the host far more
        # than on an idle stream, and 71 copies + 71 pushes outlast a delay sized by the twin's duration)
        for c in range(0, L + 7, 18):
            ys = [r.input(rows[t]) for t in range(c, min(c + 18, L + 7))]
            r.call(f"push rows {c}..", lambda: [tel.push(y) for y in ys], blocking=None if c else "lazy_create", weight=18)
        r.call("psd + gains", lambda: (tel.psd(), tel.optimise_gains(with_costs=True)))
        m = r.input(np.array([True, False, True]))
        y = r.input(rows[L + 7])
        r.call("masked reset + push + psd", lambda: (tel.reset(m), tel.push(y), tel.psd(mask=m))[2])
        blob = r.call("get_state", lambda: tel.get_state())
        b = r.input(blob)
        r.call("reset + set_state + get_state", lambda: (tel.reset(), tel.set_state(b), tel.get_state())[2], blocking="set_state")

    _both(cycles_per_ms, lambda: ModalTelemetry(B, A, length=L, device="cuda:0"), script)


def test_link(cycles_per_ms):
    from adaptive_optics_gym_amd import LinkTelemetry

    B, L = 3, 64
    rows = np.random.RandomState(7).gamma(4.0, 0.1, size=(L + 8, B)).astype(np.float32)

    def script(tel, r):
        for c in range(0, L + 7, 18):   # (18 samples per delay, as in test_telemetry)
            ps = [r.input(rows[t]) for t in range(c, min(c + 18, L + 7))]
            r.call(f"push samples {c}..", lambda: [tel.push(p) for p in ps], blocking=None if c else "lazy_create", weight=18)
        r.call("statistics", lambda: tel.statistics(q=(3.0, 6.0)), blocking="host_copy")
        m = r.input(np.array([True, False, True]))
        p = r.input(rows[L + 7])
        r.call("masked reset + push + statistics", lambda: (tel.reset(m), tel.push(p), tel.statistics(reference=0.3, mask=m))[2], blocking="host_copy")
        blob = r.call("get_state", lambda: tel.get_state())
        b = r.input(blob)
        r.call("reset + set_state + get_state", lambda: (tel.reset(), tel.set_state(b), tel.get_state())[2], blocking="set_state")
        r.call("window", lambda: tel.window(), blocking="unpack")

    _both(cycles_per_ms, lambda: LinkTelemetry(B, length=L, device="cuda:0"), script)


def test_spgd_handle(cycles_per_ms):
    """``set_params`` directly after a query that is still queued: its blocking upload must not overtake the query."""
    from adaptive_optics_gym_amd.sensorless import SPGDController

    B, A, N = 3, 8, 64
    scr = smooth_screens(B, N, 8) * 0.5
    metrics = np.random.RandomState(8).rand(5, B).astype(np.float32)

    def make():
        env = _env(B, N, act_dim=A, screens=scr, SH_operation=True, seed=5)
        return env, SPGDController(env, gain=2e-6, amplitude=[2e-8, 3e-8, 4e-8], metric="strehl", seed=2024)

    def script(h, r):
        env, ctrl = h
        r.call("reset", lambda: ctrl.reset())
        j = r.input(metrics[0])
        r.call("update", lambda: ctrl.update(j))
        j, m = r.input(metrics[1]), r.input(np.array([False, True, True]))
        r.call("masked update", lambda: ctrl.update(j, mask=m))
        j, j2 = r.input(metrics[2]), r.input(metrics[3])
        r.call("update + set_params + update", lambda: (ctrl.update(j), ctrl.set_params(gain=4e-6, amplitude=[1e-8, 2e-8, 3e-8]), ctrl.update(j2)),
               blocking="spgd_set_params")
        blob = r.call("get_state", lambda: ctrl.get_state())
        b, j = r.input(blob), r.input(metrics[4])
        r.call("reset + set_state + update", lambda: (ctrl.reset(), ctrl.set_state(b), ctrl.update(j), ctrl.get_state())[2:], blocking="set_state")

    _both(cycles_per_ms, make, script)


# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atm", ["quasi_static", "dynamic"])
def test_state_and_screens(cycles_per_ms, atm):
    torch = _torch()
    B, A, N = 7, 6, 32
    scr = smooth_screens(B, N, 3)
    new64, new32 = smooth_screens(2, N, 12), smooth_screens(1, N, 13).astype(np.float32)
    kw = dict(act_dim=A, seed=9, screen_oversampling=4)
    kw.update(dict(atm_type="dynamic", atm_vel=20.0) if atm == "dynamic" else dict(screens=scr))

    def make():
        return _env(B, N, **kw), _env(B, N, **kw)

    def script(h, r):
        env, fresh = h
        a = r.input(_acts(B, A, 1))
        r.call("reset + step", lambda: (env.reset()[0], env.step(a)))
        state = r.call("get_state", lambda: env.get_state(), blocking="get_state")
        blob = r.input(state["blob"])
        a = r.input(_acts(B, A, 2))
        r.call("set_state into a fresh handle + step", lambda: (fresh.set_state(dict(state, blob=blob)), fresh.step(a), fresh.get_screens())[1:],
               blocking="set_state")
        a = r.input(_acts(B, A, 2))
        r.call("the same step on the source", lambda: (env.step(a), env.get_screens()))
        s64, s32 = r.input(new64), r.input(new32)
        r.call("set_screens(first=5)", lambda: (env.set_screens(s64, first=5), env.set_screens(s32, first=2), env.get_screens())[2], blocking="set_screens")
        act = r.call("get_actuators", lambda: env.get_actuators())
        v = r.input(act * 0.5)
        a = r.input(_acts(B, A, 3))
        r.call("set_actuators + get_actuators + step", lambda: (env.set_actuators(v), env.get_actuators(), env.step(a))[1:], blocking="set_actuators")

    _both(cycles_per_ms, make, script)


def test_two_handles_two_streams(cycles_per_ms):
    """A batch of 33 as halves of 16 + 17 (``global_env_offset``) on two side streams, submitted alternately with no synchronisation in
    between, against the whole batch on the default stream: semi_dynamic device screens plus a detector."""
    torch = _torch()
    B, A, N, T = 33, 6, 64, 3
    kw = dict(act_dim=A, atm_type="semi_dynamic", seed=3, obs_photons=1e4, obs_read_noise=2.0, timesteps_per_episode=T)
    acts = [torch.from_numpy(_acts(B, A, t)).cuda() for t in range(T)]
    whole = _env(B, N, **kw)
    parts = [(0, 16), (16, 33)]
    streams = [sh.side_stream(torch, cycles_per_ms), sh.side_stream(torch, cycles_per_ms)]
    halves = []
    try:
        want = [whole.reset()[0].clone()] + [sh._clone(torch, whole.step(a)) for a in acts] + [whole.reset()[0].clone()]
        for (lo, hi), s in zip(parts, streams):
            with torch.cuda.stream(s):
                halves.append(_env(hi - lo, N, global_env_offset=lo, total_envs=B, **kw))
        real = [[a[lo:hi].contiguous() for a in acts] for lo, hi in parts]
        ins = [[torch.full_like(a, float("nan")) for a in row] for row in real]
        torch.cuda.synchronize()
        got = [[], []]
        events = []
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                torch.cuda._sleep(int(cycles_per_ms * 2 * (T + 2) * sh.FLOOR_MS))   # (every call of both handles is behind each producer)
                for d, v in zip(ins[i], real[i]):
                    d.copy_(v, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(s)
                events.append(ev)
        t_ev = time.perf_counter()
        for step in range(T + 2):
            for i, s in enumerate(streams):
                with torch.cuda.stream(s):
                    e = halves[i]
                    got[i].append(e.reset()[0].clone() if step in (0, T + 1) else sh._clone(torch, e.step(ins[i][step - 1])))
        queued = [not ev.query() for ev in events]
        print(f"\n[streams] two streams: {1e3 * (time.perf_counter() - t_ev):.2f} ms of host time behind {2 * (T + 2) * sh.FLOOR_MS:.0f} ms delays")
        torch.cuda.synchronize()
        assert all(queued), "the producers had finished when the last call returned: the delay is too short or a call blocked"
        lines = []
        for k, w in enumerate(want):
            fw, f0, f1 = [], [], []
            sh._flatten(torch, w, f"call{k}", fw)
            sh._flatten(torch, got[0][k], "", f0)
            sh._flatten(torch, got[1][k], "", f1)
            for (path, x), (_, y0), (_, y1) in zip(fw, f0, f1):
                if not sh.same(torch, torch.cat([y0, y1]), x):
                    lines.append(f"{path}: the two halves on two streams differ from the whole batch on the default stream")
        assert not lines, "\n".join(lines)
    finally:
        torch.cuda.synchronize()
        _close([whole] + halves)
