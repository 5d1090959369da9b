"""The layered atmosphere on the device: aog_evolve_atmosphere, aog_install_layer_sum (k_layer_mean, k_layer_sum_tiles, k_layer_sum_f64)
and ``LayeredAOEnv`` on top of them.

Shapes are the smallest that reach the kernels' edges: N = 32 and 48 (n_ap no multiple of 64: the last pair of pixel tiles is half
empty or half padding), B = 37 and 70 (a partial last env tile; three env tiles and a fourth of padding), 1 .. 3 layers, 4 .. 6 steps at
winds of 30 .. 70 m/s (2 .. 7 pixels per step: the ring origins are non-zero and differ per layer, env and axis)."""
import ctypes as C

import numpy as np
import pytest

import layered_reference as ref
from helpers import ScriptedRNG, device_mode_stencil_draws
from test_gpu_parity import RTOL, _assert_obs_close, _torch

pytestmark = pytest.mark.gpu

FRACTIONS = {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.3, 0.2]}
SPEEDS = [30.0, 50.0, 70.0]


def _layers(L):
    return [{"fraction": f, "speed": v} for f, v in zip(FRACTIONS[L], SPEEDS)]


def _kw(N=32, A=6, T=5, **more):
    kw = dict(act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T, num_pupil_pixels=N, verbose=False)
    kw.update(more)
    return kw


def _layered(B, L, seed=11, r0=0.15, **kw):
    from adaptive_optics_gym_amd import LayeredAOEnv

    return LayeredAOEnv(B, "cuda:0", atm_layers=_layers(L), atm_fried=r0, seed=seed, **_kw(**kw))


def _actions(torch, T, B, A, seed=5):
    g = torch.Generator("cuda").manual_seed(seed)
    return torch.randn((T, B, A), device="cuda", generator=g) * 0.5 ** 0.5


def _noise_for(torch, env, gen):
    """Normals for the coming extrusions of a dynamic env ([B, max_ext, N]) and how many rows each env consumes."""
    from adaptive_optics_gym_amd.atmosphere_host import integer_shifts

    shifts = integer_shifts(env.velocity_vectors, env.timestep * env.delta_t, (env.timestep + 1) * env.delta_t, env.params.pupil_pixel)
    counts = np.abs(shifts).sum(axis=1)
    assert counts.max() >= 1
    return torch.randn((env.num_envs, int(counts.max()), env.num_pupil_pixels), device="cuda", dtype=torch.float64, generator=gen), counts, shifts


def _step_tensors(ret):
    obs, rew, done, _, info = ret
    return [obs.clone(), rew.clone(), done.clone(), info["obs_raw"].clone(), info["power"].clone(), info["strehl"].clone()]


# ---- 1. evolve is the step's atmosphere ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_normals", [False, True], ids=["device_stream", "host_normals"])
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_evolve_is_the_atmosphere_half_of_a_step(extrusion, host_normals):
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A, k = 37, 32, 8, 5
    mk = lambda: BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=45, atm_fried=0.15, seed=3, extrusion=extrusion, **_kw(N=N, A=A, T=k))
    stepped, evolved = mk(), mk()
    acts = _actions(torch, k, B, A)
    gen = torch.Generator("cuda").manual_seed(9)
    assert torch.equal(stepped.get_screens(), evolved.get_screens())
    stepped.reset()
    start = stepped.get_screens().clone()
    for t in range(k):
        if host_normals:
            noise, _, _ = _noise_for(torch, stepped, gen)
            stepped.set_extrusion_noise(noise)
            evolved.set_extrusion_noise(noise)
        stepped.step(acts[t])
        evolved.evolve_atmosphere()
        assert evolved.timestep == stepped.timestep == t + 1
        assert torch.equal(stepped.get_screens(), evolved.get_screens()), f"step {t}"
    assert not torch.equal(start, evolved.get_screens())
    assert stepped.device_status() == 0 and evolved.device_status() == 0
    stepped.close(), evolved.close()


# ---- 2. install against the host restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,L", [(32, 37, 2), (48, 70, 3), (32, 70, 1), (48, 37, 2)])
def test_install_matches_the_host_restatement(N, B, L):
    """fp32 tiles of the front = float32 of the float64 restatement from the layers' own screens, to one fp32 ulp of the value (the mean's
    float64 summation order is the only freedom: <= n_ap 2^-53 max|s| on a value, far below half an fp32 ulp except where it tips a rounding);
    pad pixels and pad envs exactly zero."""
    torch = _torch()
    from adaptive_optics_gym_amd.atmosphere_host import integer_shifts

    env = _layered(B, L, N=N)
    acts = _actions(torch, 4, B, 6)
    env.reset()
    for t in range(4):
        env.step(acts[t])
    # the rings have turned: whole-pixel shifts that differ per layer and per axis
    total = [integer_shifts(v, 0.0, 4 * env.delta_t, env.params.pupil_pixel) for v in env.velocity_vectors]
    assert all(np.abs(s).max(axis=1).min() >= 4 for s in total)
    assert L == 1 or not np.array_equal(total[0], total[1])
    assert env.velocity_vectors.shape == (L, B, 2) and env.num_layers == L
    screens = [env.layer_screens(i).cpu().numpy() for i in range(L)]
    ap = np.asarray(env.tables.ap_index)
    n_ap = ap.size
    assert n_ap % 64 != 0
    want = ref.install(screens, [np.zeros((B, 2), dtype=int)] * L, ap, N, env.wavelength_wfs)
    got = ref.front_store(env)
    assert got.shape == want["tiles"].shape
    rev, pad_nonzero = ref.unpack_tiles(got, B, n_ap)
    assert pad_nonzero == 0
    err = np.abs(rev.astype(np.float64) - want["rev"].astype(np.float64))
    ulp = np.spacing(np.abs(want["rev"])).astype(np.float64)
    print(f"N={N} B={B} L={L}: {np.count_nonzero(err)} of {err.size} values differ, worst {np.max(err / ulp):.2f} ulp")
    assert np.all(err <= ulp)
    # the env's float64 sum is the same sum
    np.testing.assert_array_equal(env.get_screens().cpu().numpy().reshape(B, -1)[:, ap], want["s"])
    env.close()


def test_install_into_a_float64_front():
    """precision='fp64': the front's float64 screens are s - mean within 1e-13 of the screen's scale (the order of the mean's additions:
    <= n_ap 2^-53 max|s| ~ 1e-13 max|s| at n_ap ~ 800)."""
    torch = _torch()
    B, N, L = 37, 32, 3
    env = _layered(B, L, N=N, precision="fp64")
    acts = _actions(torch, 4, B, 6)
    env.reset()
    for t in range(4):
        env.step(acts[t])
    screens = [env.layer_screens(i).cpu().numpy() for i in range(L)]
    want = ref.install(screens, [np.zeros((B, 2), dtype=int)] * L, np.asarray(env.tables.ap_index), N, env.wavelength_wfs)
    got = ref.front_store(env, fp64=True)
    scale = np.abs(want["psi64"]).max()
    print(f"float64 front: max error {np.abs(got - want['psi64']).max() / scale:.2e} of the screen's scale")
    np.testing.assert_allclose(got, want["psi64"], rtol=0, atol=1e-13 * scale)
    env.close()


# ---- 3. one layer is today's dynamic env ---------------------------------------------------------------------------------------------------
def test_one_layer_anchors_to_the_plain_dynamic_env():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    B, N, A, T = 37, 32, 6, 5
    lay = LayeredAOEnv(B, "cuda:0", atm_layers=[{"fraction": 1.0, "speed": 45}], atm_fried=0.15, seed=21, **_kw(N=N, A=A, T=T))
    plain = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=45, atm_fried=0.15, seed=21, **_kw(N=N, A=A, T=T))
    np.testing.assert_array_equal(lay.velocity_vectors[0], plain.velocity_vectors)
    acts = _actions(torch, 2 * T, B, A)
    for ep in range(2):
        lay.reset(), plain.reset()
        assert torch.equal(lay.get_screens(), plain.get_screens())
        _assert_obs_close(lay.last_obs_raw.double().cpu().numpy(), plain.last_obs_raw.double().cpu().numpy())
        for t in range(T):
            a = acts[ep * T + t]
            o1, r1, d1, _, i1 = lay.step(a)
            o2, r2, d2, _, i2 = plain.step(a)
            assert torch.equal(lay.get_screens(), plain.get_screens()), f"episode {ep} step {t}"
            _assert_obs_close(i1["obs_raw"].double().cpu().numpy(), i2["obs_raw"].double().cpu().numpy())
            np.testing.assert_allclose(i1["power"].cpu().numpy(), i2["power"].cpu().numpy(), rtol=RTOL)
            np.testing.assert_allclose(i1["strehl"].cpu().numpy(), i2["strehl"].cpu().numpy(), rtol=RTOL)
            assert torch.equal(d1, d2) and bool(d1.all()) == (t == T - 1)
    assert lay.timestep == plain.timestep == 2 * T
    lay.close(), plain.close()


# ---- 4. oracle parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,extrusion", [(2, "auto"), (3, "auto"), (2, "f64"), (3, "f64")])
def test_layered_env_matches_the_oracle(L, extrusion):
    """test_config4's recipe: the extrusion normals handed to every layer are replayed through one oracle InfiniteAtmosphericLayer per layer
    and sampled env; the summed screen goes through the oracle's optics.  Screens: 1e-6 rad absolute on the int8 extrusion, rtol 1e-9 on the
    float64 one; observations, power and Strehl 1e-5 relative."""
    torch = _torch()
    from oracle.ao_env_oracle import AOEnvOracle

    B, N, A, T, seed, r0 = 37, 32, 6, 5, 17, 0.15
    env = _layered(B, L, seed=seed, r0=r0, N=N, A=A, T=T, extrusion=extrusion)
    from adaptive_optics_gym_amd.layered import layer_seed

    okw = dict(act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T, num_pupil_pixels=N, verbose=False)
    ids = [0, B // 2 - 1, B - 1]
    lay_ref = {}
    for b in ids:
        for i, lay in enumerate(env.layers):
            geo = device_mode_stencil_draws(1234 if layer_seed(seed, i) is None else layer_seed(seed, i), B, N)
            rng = ScriptedRNG(lay.wind_u[b], [g.copy() for g in geo])
            o = AOEnvOracle(atm_type="dynamic", atm_vel=SPEEDS[i], atm_fried=r0 * FRACTIONS[L][i] ** (-3.0 / 5.0),
                            screen=lay.get_screens(b, 1)[0].cpu().numpy().ravel(), rng=rng, **okw)
            np.testing.assert_allclose(o.layer.velocity, lay.velocity_vectors[b], rtol=1e-14)
            lay_ref[b, i] = o
    total = lambda b: sum(lay_ref[b, i].layer._achromatic_screen for i in range(L))
    optics = {b: AOEnvOracle(atm_type="quasi_static", atm_fried=r0, screen=total(b).copy(), **okw) for b in ids}
    env.reset()
    for b in ids:
        optics[b].reset()
        _assert_obs_close(env.last_obs_raw[b].double().cpu().numpy(), optics[b].last_obs_raw)
    acts = _actions(torch, T, B, A)
    gen = torch.Generator("cuda").manual_seed(99)
    worst = 0.0
    for t in range(T):
        fed = []
        for lay in env.layers:
            noise, counts, _ = _noise_for(torch, lay, gen)
            lay.set_extrusion_noise(noise)
            fed.append((noise, counts))
        obs, rew, done, _, info = env.step(acts[t])
        for b in ids:
            for i, lay in enumerate(env.layers):
                o = lay_ref[b, i]
                o.rng.normals.extend(fed[i][0][b, :int(fed[i][1][b])].cpu().numpy())
                o.timestep += 1
                o.layer.t = o.timestep * o.delta_t
                assert not o.rng.normals
                got, want = lay.get_screens(b, 1)[0].cpu().numpy().ravel(), o.layer._achromatic_screen
                if extrusion == "f64":
                    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
                else:
                    err = float(np.abs(got - want).max()) / 1.5e-6
                    worst = max(worst, err)
                    assert err < 1e-6, f"step {t}, env {b}, layer {i}: screen error {err:.2e} rad"
            optics[b].layer._achromatic_screen = total(b).copy()
            _, r_rew, r_done, _, r_info = optics[b].step(acts[t, b].cpu().numpy())
            _assert_obs_close(info["obs_raw"][b].double().cpu().numpy(), optics[b].last_obs_raw)
            np.testing.assert_allclose(float(info["power"][b]), r_info["power"], rtol=RTOL)
            np.testing.assert_allclose(float(info["strehl"][b]), optics[b].last_strehl, rtol=RTOL)
            np.testing.assert_allclose(float(rew[b]), r_rew, rtol=0, atol=100 * RTOL)
            assert bool(done[b]) == r_done
    print(f"L={L} {extrusion}: worst layer screen error {worst:.2e} rad")
    env.close()


# ---- 5. split batch --------------------------------------------------------------------------------------------------------------------------
def test_split_batch_reproduces_the_whole_batch():
    torch = _torch()
    B, N, A, T, L = 70, 32, 6, 4, 2
    whole = _layered(B, L, N=N, A=A, T=T, total_envs=B)
    halves = [_layered(35, L, N=N, A=A, T=T, global_env_offset=off, total_envs=B) for off in (0, 35)]
    acts = _actions(torch, T, B, A)
    cat = lambda xs: torch.cat(list(xs), dim=0)
    ow, _ = whole.reset()
    oh = cat(h.reset()[0] for h in halves)
    assert torch.equal(ow, oh) and torch.equal(whole.get_screens(), cat(h.get_screens() for h in halves))
    for t in range(T):
        rw = _step_tensors(whole.step(acts[t]))
        rh = [_step_tensors(h.step(acts[t, off:off + 35].contiguous())) for h, off in zip(halves, (0, 35))]
        for k, x in enumerate(rw):
            assert torch.equal(x, cat(r[k] for r in rh)), f"step {t}, output {k}"
        assert torch.equal(whole.get_screens(), cat(h.get_screens() for h in halves))
    ow, _ = whole.reset()
    assert torch.equal(ow, cat(h.reset()[0] for h in halves))
    whole.close()
    for h in halves:
        h.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------------------------
def test_state_restore_resumes_bit_identically():
    torch = _torch()
    B, N, A, T, L = 37, 32, 6, 6, 2
    env = _layered(B, L, N=N, A=A, T=T)
    acts = _actions(torch, T, B, A)
    env.reset()
    for t in range(2):
        env.step(acts[t])
    state = env.get_state()
    assert len(state["layers"]) == L
    first = [_step_tensors(env.step(acts[t])) + [env.get_screens().clone()] for t in range(2, 5)]
    env.set_state(state)
    assert env.timestep == 2 and all(lay.timestep == 2 for lay in env.layers)
    again = [_step_tensors(env.step(acts[t])) + [env.get_screens().clone()] for t in range(2, 5)]
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    # a second env built alike resumes from the same state too
    other = _layered(B, L, N=N, A=A, T=T)
    other.set_state(state)
    third = [_step_tensors(other.step(acts[t])) + [other.get_screens().clone()] for t in range(2, 5)]
    for a, b in zip(first, third):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    with pytest.raises(ValueError, match="layers"):
        other.set_state({**state, "layers": state["layers"][:1]})
    env.close(), other.close()


# ---- 7. riders ---------------------------------------------------------------------------------------------------------------------------------
def test_everything_that_reads_the_screens_works_on_the_front():
    """wavefront_truth, the science camera and output_gradient on a 2-layer env equal, bit for bit, those of a quasi-static twin handle given
    the same layer list; lookahead is refused politely, set_screens loudly."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A, T, L = 37, 32, 8, 4, 2
    env = _layered(B, L, N=N, A=A, T=T, science_window=8)
    twin = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_fried=0.15, seed=11, tables=env.tables, science_window=8,
                        screens=np.zeros((B, N, N)), **_kw(N=N, A=A, T=T))
    acts = _actions(torch, 2, B, A)
    env.reset(), twin.reset()
    for t in range(2):
        r1 = _step_tensors(env.step(acts[t]))
        twin.install_layer_sum(env.layers)
        r2 = _step_tensors(twin.step(acts[t]))
        for x, y in zip(r1, r2):
            assert torch.equal(x, y)
        for e in (env, twin):
            e.science_integrate()
    w1, w2 = env.wavefront_truth(), twin.wavefront_truth()
    for k in w1:
        assert torch.equal(w1[k], w2[k]), k
    assert float(w1["rms"].min()) > 0
    s1, s2 = env.science_exposure(), twin.science_exposure()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert int(s1["frames"].min()) == 2
    one = torch.ones(B, dtype=torch.float64, device="cuda")
    g1, v1 = env.output_gradient(g_strehl=one, g_power=one, with_values=True)
    g2, v2 = twin.output_gradient(g_strehl=one, g_power=one, with_values=True)
    assert torch.equal(g1, g2) and torch.equal(v1, v2) and float(g1.abs().max()) > 0
    assert torch.equal(env.phase_screen(B - 1), twin.phase_screen(B - 1)) and float(env.phase_screen(0).abs().max()) > 0
    assert env.lookahead(True) is False
    with pytest.raises(RuntimeError, match="sum of the layers"):
        env.set_screens(np.zeros((B, N, N)))
    env.close(), twin.close()


def test_fused_policy_rollout_equals_the_unfused_loop():
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, make_actor, rollout

    B, N, A, T, L = 37, 32, 8, 4, 2
    torch.manual_seed(3)
    actor = make_actor(4, A, 32, device="cuda:0")
    outs = []
    for fused in (False, True):
        env = _layered(B, L, N=N, A=A, T=T)
        outs.append(rollout(env, actor, episodes=2, actor_impl="hip", dev_actor=DeviceActor(actor, seed=10), fused_policy=fused))
        assert env.timestep == 2 * T
        env.close()
    compared = 0
    for k, v in outs[0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, outs[1][k]), k
            compared += 1
        elif isinstance(v, np.ndarray):
            np.testing.assert_array_equal(v, outs[1][k])
    assert compared >= 4 and tuple(outs[0]["obs"].shape[-2:]) == (B, 4)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_front_usable():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A, T = 37, 32, 6, 4
    env = _layered(B, 2, N=N, A=A, T=T)
    front_kw = dict(atm_type="quasi_static", atm_fried=0.15, seed=11, screens=np.zeros((B, N, N)))
    lib, s = env.lib, env._stream()

    def install(dst, layers, n=None):
        arr = (C.c_void_p * max(1, len(layers)))(*[x._handle.value for x in layers])
        return lib.aog_install_layer_sum(dst._handle, arr, len(layers) if n is None else n, s), lib.aog_last_error().decode()

    before = ref.front_store(env).copy()
    dyn = env.layers[0]
    static = BatchedAOEnv(B, "cuda:0", tables=env.tables, **front_kw, **_kw(N=N, A=A, T=T))
    small = BatchedAOEnv(B - 5, "cuda:0", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, **_kw(N=N, A=A, T=T))
    other_n = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, **_kw(N=48, A=A, T=T))
    shifted = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, global_env_offset=5, **_kw(N=N, A=A, T=T))
    valu = BatchedAOEnv(B, "cuda:0", kernel="valu", **front_kw, **_kw(N=N, A=A, T=T))
    for dst, layers, n, code, word in ((dyn, [env.layers[1]], None, -1, "atm_dynamic"), (env, [static], None, -1, "not a dynamic handle"),
                                       (env, [dyn, small], None, -1, "does not match"), (env, [other_n], None, -1, "does not match"),
                                       (env, [shifted], None, -1, "does not match"), (env, [], 0, -1, "0 layers"),
                                       (env, [dyn] * 9, None, -1, "9 layers"), (valu, list(env.layers), None, -4, "VALU")):
        rc, msg = install(dst, layers, n)
        assert rc == code and word in msg and "aog_install_layer_sum" in msg, (rc, msg)
    if torch.cuda.device_count() > 1:   # a layer on another device
        far = BatchedAOEnv(B, "cuda:1", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, **_kw(N=N, A=A, T=T))
        rc, msg = install(env, [far])
        assert rc == -1 and "does not match" in msg
        far.close()
    # evolve: not on a static handle, not with lookahead on
    assert lib.aog_evolve_atmosphere(static._handle, s) == -3 and b"atm_dynamic" in lib.aog_last_error()
    assert small.lookahead(True) is True
    t0 = small.timestep
    assert lib.aog_evolve_atmosphere(small._handle, s) == -3 and b"aog_set_lookahead" in lib.aog_last_error()
    with pytest.raises(RuntimeError, match="aog_evolve_atmosphere"):
        small.evolve_atmosphere()
    assert small.timestep == t0
    small.lookahead(False)
    small.evolve_atmosphere()
    with pytest.raises(RuntimeError, match="dynamic"):
        static.evolve_atmosphere()
    # nothing was written, and the front still steps
    np.testing.assert_array_equal(ref.front_store(env), before)
    env.reset()
    obs, rew, done, _, info = env.step(_actions(torch, 1, B, A)[0])
    assert bool(torch.isfinite(info["obs_raw"]).all()) and 0 <= float(info["strehl"].min()) <= float(info["strehl"].max()) <= 1
    assert env.device_status() == 0
    for e in (env, static, small, other_n, shifted, valu):
        e.close()
