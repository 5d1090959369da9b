"""Layer altitudes and sightlines on the device: aog_install_layer_sum_sightline (the SightLayers form of k_layer_mean,
k_layer_sum_tiles and k_layer_sum_f64) against the host restatement (tests/sightline_reference.py), anchored to the two existing installations, and
``LayeredAOEnv(layer_altitudes=...)`` / ``add_sightline`` on top of it.

Shapes follow test_gpu_layered.py, for its reasons: N = 32 under a meta-pupil of N_L = 48 (margin c = 8; n_ap no multiple of 64: the last
pair of pixel tiles is half empty), B in {1, 33} (one env; one env past a 32-env tile), L in {1, 3}, A = 6 Zernike modes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import checkpoint_harness as ch
import disturbance_reference as dref
import layered_reference as lref
import sightline_reference as ref
from test_gpu_disturbance import _static_env, _upload
from test_gpu_layered import _actions, _kw, _layers, _step_tensors
from test_gpu_streams import _acts, _both, cycles_per_ms  # noqa: F401  (cycles_per_ms: the module's calibration fixture)
from test_gpu_parity import _torch

pytestmark = pytest.mark.gpu

# entry point (include/aogym_sightline.h, every one with a `void* stream`) -> the test here that drives it on a caller's side stream
COVERED = {"aog_install_layer_sum_sightline": "test_the_entry_point_runs_on_a_side_stream"}

N, NL = 32, 48
MARGIN = (NL - N) // 2
PITCH = 0.5 / N
ALTITUDES = np.array([1e4, 2e3, 6e3])


def _meta_params(n=NL):
    from adaptive_optics_gym_amd import OpticalParams

    return dataclasses.replace(OpticalParams(num_pupil_pixels=N), num_pupil_pixels=n, telescope_diameter=0.5 * n / N)


@pytest.fixture(scope="module")
def layer_sets():
    """Per (N_l, B): three evolved dynamic layers at the front's pixel pitch whose rings have turned on both axes (shared by every case;
    nothing below changes them)."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.atmosphere_host import integer_shifts

    sets = {}
    for n, B in ((NL, 1), (NL, 33), (N, 33)):
        lays = [BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30.0 + 20.0 * i, atm_fried=0.15, seed=3 + i, params=_meta_params(n), **_kw(N=n, T=0))
                for i in range(3)]
        for lay in lays:
            for _ in range(3):
                lay.evolve_atmosphere()
            assert abs(lay.params.pupil_pixel - PITCH) < 1e-15
            turned = np.abs(integer_shifts(lay.velocity_vectors, 0.0, 3 * lay.delta_t, PITCH))
            assert turned.max() >= 1 and (B == 1 or (turned.max(axis=0) >= 1).all())      # (B = 33: envs with a turned ring on either axis)
        sets[n, B] = lays
    torch.cuda.synchronize()
    yield sets
    for lays in sets.values():
        for lay in lays:
            lay.close()


def _install(front, layers, shifts, coeff=None):
    handles = (C.c_void_p * max(1, len(layers)))(*[lay._handle.value for lay in layers])
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    rc = front.lib.aog_install_layer_sum_sightline(front._handle, handles, len(layers), shifts.ctypes.data_as(C.c_void_p),
                                                   None if coeff is None else C.c_void_p(coeff.data_ptr()), 0 if coeff is None else int(coeff.shape[1]),
                                                   front._stream())
    return rc, front.lib.aog_last_error().decode()


def _shifts(B, L, seed=0):
    """[L, B, 2] through the package's own formula: per-env angles of both signs, a different altitude per layer, the largest shift exactly
    the margin's c - 1 (the highest layer: +(c - 1) in x beside a negative fraction in y for env 0, -(c - 1) and +(c - 1) for env 1)."""
    from adaptive_optics_gym_amd.layered import sightline_shifts

    unit = np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 2))
    unit[0] = (1.0, -0.37)
    unit[1:2] = (-1.0, 1.0)
    s = sightline_shifts(ALTITUDES[:L], unit, 1.0) / ALTITUDES[0] * (MARGIN - 1)
    assert np.abs(s).max() == MARGIN - 1 and (s > 0).any() and (s < 0).any() and (s != np.floor(s)).any()
    return s


def _blob(front):
    from adaptive_optics_gym_amd import BatchedAOEnv

    return BatchedAOEnv.get_state(front)["blob"].cpu().numpy().copy()


# ---- 1. install against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fp64"])
@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("B", [1, 33])
def test_install_matches_the_host_restatement(layer_sets, B, L, K, precision):
    """float64 front: psi64 bit for bit.  Fast front: the standard of test_gpu_layered.test_install_matches_the_host_restatement — one fp32
    ulp of the value, pad pixels and pad envs exact zeros."""
    torch = _torch()
    layers = layer_sets[NL, B][:L]
    front = _static_env(B, N=N, precision=precision)
    ap = np.asarray(front.tables.ap_index)
    n_ap = ap.size
    assert n_ap % 64 != 0
    shifts = _shifts(B, L, seed=10 * L + B)
    rng = np.random.RandomState(100 * K + L)
    basis, coeff, cdev = None, None, None
    if K:
        basis, coeff = rng.randn(K, n_ap) * 2 * np.pi, rng.randn(B, K) * 1e-7
        assert _upload(front, basis)[0] == 0
        cdev = torch.from_numpy(coeff).cuda()
    rc, msg = _install(front, layers, shifts, cdev)
    assert rc == 0, msg
    fp64 = precision == "fp64"
    got = lref.front_store(front, fp64=fp64)
    screens = [lay.get_screens().cpu().numpy() for lay in layers]
    want = ref.install(screens, shifts, ap, N, front.wavelength_wfs, coeff, basis)
    if fp64:
        np.testing.assert_array_equal(got, want["psi64"])
    else:
        assert got.shape == want["tiles"].shape
        rev, pad_nonzero = lref.unpack_tiles(got, B, n_ap)
        assert pad_nonzero == 0
        err = np.abs(rev.astype(np.float64) - want["rev"].astype(np.float64))
        ulp = np.spacing(np.abs(want["rev"])).astype(np.float64)
        print(f"B={B} L={L} K={K}: {np.count_nonzero(err)} of {err.size} values differ, worst {np.max(err / ulp):.2f} ulp")
        assert np.all(err <= ulp)
    # the displacement and the terms are there: the on-axis sum of the same layers differs
    on_axis = ref.sightline_sum(screens, np.zeros_like(shifts), ap, N)
    assert np.abs(want["s"] - on_axis).max() > 1e-8
    # the same shifts again (the front's buffer is reused) leave the same bits; other shifts other bits
    before = _blob(front)
    assert _install(front, layers, shifts, cdev)[0] == 0
    np.testing.assert_array_equal(_blob(front), before)
    assert _install(front, layers, -shifts, cdev)[0] == 0
    assert not np.array_equal(_blob(front), before)
    front.close()


# ---- 2. anchor to the existing path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_zero_shifts_on_the_pupil_leave_the_existing_installations_bits(layer_sets, precision):
    torch = _torch()
    B, L, K = 33, 2, 2
    layers = layer_sets[N, B][:L]
    front = _static_env(B, N=N, precision=precision)
    zero = np.zeros((L, B, 2))
    rc, msg = _install(front, layers, zero)
    assert rc == 0, msg
    new = _blob(front)
    front.install_layer_sum(layers)
    np.testing.assert_array_equal(new, _blob(front))
    assert np.abs(lref.front_store(front, fp64=precision == "fp64")).max() > 0
    # and with a two-term disturbance, against aog_install_layer_sum_disturbed
    rng = np.random.RandomState(4)
    assert _upload(front, rng.randn(K, int(front.tables.n_ap)) * 2 * np.pi)[0] == 0
    cdev = torch.from_numpy(rng.randn(B, K) * 1e-7).cuda()
    rc, msg = _install(front, layers, zero, cdev)
    assert rc == 0, msg
    new_dist = _blob(front)
    assert not np.array_equal(new_dist, new)
    handles = (C.c_void_p * L)(*[lay._handle.value for lay in layers])
    assert front.lib.aog_install_layer_sum_disturbed(front._handle, handles, L, C.c_void_p(cdev.data_ptr()), K, front._stream()) == 0
    np.testing.assert_array_equal(new_dist, _blob(front))
    front.close()


# ---- 3. integer shifts are translations --------------------------------------------------------------------------------------------------------
def test_integer_shifts_are_translations(layer_sets):
    """One layer, shift (3, -2): every value the front is left with is the layer's logical screen three pixels right and two up, exactly —
    psi64 = t - mean(t) bit for bit (t the translated screen, its mean in the fixed order), and psi64 + mean gives t back to one rounding."""
    B = 33
    layer = layer_sets[NL, B][0]
    front = _static_env(B, N=N, precision="fp64")
    shifts = np.tile(np.array([3.0, -2.0]), (1, B, 1))
    rc, msg = _install(front, [layer], shifts)
    assert rc == 0, msg
    ap = np.asarray(front.tables.ap_index)
    iy, ix = np.divmod(ap, N)
    screen = layer.get_screens().cpu().numpy()
    t = screen[:, iy + MARGIN - 2, ix + MARGIN + 3]
    mean = dref.mean_in_fixed_order(t)
    got = lref.front_store(front, fp64=True)
    np.testing.assert_array_equal(got, t - mean[:, None])
    np.testing.assert_allclose(got + mean[:, None], t, rtol=0, atol=2.0 ** -52 * np.abs(t).max())
    assert np.abs(t - screen[:, iy + MARGIN, ix + MARGIN]).max() > 1e-8
    front.close()


# ---- 4. sightlines through the env -------------------------------------------------------------------------------------------------------------
def _layered(B, L=2, altitudes=(0.0, 1e4), seed=11, **kw):
    from adaptive_optics_gym_amd import LayeredAOEnv

    return LayeredAOEnv(B, "cuda:0", atm_layers=_layers(L), atm_fried=0.15, seed=seed, layer_altitudes=list(altitudes), **_kw(**kw))


def _sight(info, name):
    s = info["sightlines"][name]
    return [s["obs"], s["reward"], s["power"], s["strehl"]]


def test_a_sightline_at_the_envs_own_angle_sees_what_the_env_sees():
    torch = _torch()
    B, A, T = 33, 6, 5
    theta = (5e-6, -3e-6)       # 3.2 and 1.9 pixels at 10 km
    env = _layered(B, A=A, T=T, field_angle=theta, sightlines={"same": theta, "axis": (0.0, 0.0)})
    assert env.meta_pupil_pixels == 44 and list(env.layer_margins) == [0, 6] and [lay.num_pupil_pixels for lay in env.layers] == [32, 44]
    assert env.layers[0].tables is env.tables and env.layers[1].tables is not env.tables
    assert abs(env.layers[1].params.pupil_pixel - env.params.pupil_pixel) < 1e-15
    same, axis = env.sightlines["same"], env.sightlines["axis"]
    acts = _actions(torch, 2 * T, B, A)
    differ = 0
    for ep in range(2):
        obs, _ = env.reset()
        assert torch.equal(obs, same.env._last_obs) and not torch.equal(obs, axis.env._last_obs)
        for t in range(T):
            o, r, d, _, info = env.step(acts[ep * T + t])
            for x, y, z in zip([o, r, info["power"], info["strehl"]], _sight(info, "same"), _sight(info, "axis")):
                assert torch.equal(x, y), f"episode {ep} step {t}"
                differ += int(not torch.equal(x, z))
            assert bool(d.all()) == (t == T - 1) and same.last is info["sightlines"]["same"]
    assert differ == 2 * T * 4     # with a layer at 10 km the on-axis front sees another wavefront, every step and in every output
    # what the fronts carry is the instruments' to read
    assert torch.equal(env.wavefront_truth()["rms"], same.env.wavefront_truth()["rms"])
    # fused stepping is refused with its reason; the angle moves inside the margin only
    with pytest.raises(RuntimeError, match="sightlines attached"):
        env.step_with_spgd(None)
    with pytest.raises(RuntimeError, match="sightlines attached"):
        env.step_with_policy(None)
    with pytest.raises(ValueError, match="leaves 5"):
        axis.set_angle((0.0, 1e-5))
    with pytest.raises(ValueError, match="leaves 5"):
        env.set_field_angle((-1e-5, 0.0))
    with pytest.raises(ValueError, match="already"):
        env.add_sightline((0.0, 0.0), "axis")
    np.testing.assert_array_equal(axis.angle, np.zeros((B, 2)))
    axis.set_angle(theta)
    env.reset()
    _, _, _, _, info = env.step(acts[0])
    for y, z in zip(_sight(info, "same"), _sight(info, "axis")):
        assert torch.equal(y, z)
    assert env.device_status() == 0
    env.close()
    assert not env.sightlines


def test_a_layer_at_altitude_zero_contributes_identically_to_both_fronts():
    """That layer installed alone: whatever the angle, the sightline's front and the env's step to the same bits."""
    torch = _torch()
    B, A, T = 33, 6, 3
    env = _layered(B, L=1, altitudes=(0.0,), A=A, T=T, meta_pupil_pixels=NL, sightlines={"far": (4e-4, -2e-4)})
    assert list(env.layer_margins) == [0] and env.layers[0].num_pupil_pixels == N
    plain = __import__("adaptive_optics_gym_amd").LayeredAOEnv(B, "cuda:0", atm_layers=_layers(1), atm_fried=0.15, seed=11, **_kw(A=A, T=T))
    acts = _actions(torch, T, B, A)
    env.reset(), plain.reset()
    for t in range(T):
        o, r, d, _, info = env.step(acts[t])
        po, pr, _, _, pinfo = plain.step(acts[t])
        for x, y, z in zip([o, r, info["power"], info["strehl"]], _sight(info, "far"), [po, pr, pinfo["power"], pinfo["strehl"]]):
            assert torch.equal(x, y) and torch.equal(x, z)      # (and the env without altitudes: the pupil-plane path computes the same)
    env.close(), plain.close()


# ---- 5. bits survive ---------------------------------------------------------------------------------------------------------------------------
DIST = dict(shapes=["tip", "focus"], vibrations=[dict(term=0, frequency=30.0, damping=0.02, rms=4e-8)], static=[0.0, -3e-8])


def test_split_batch_reproduces_the_whole_batch():
    torch = _torch()
    B, A, T = 66, 6, 3
    g = np.arange(B)
    angles = np.stack([4e-6 * np.cos(g), 4e-6 * np.sin(g)], axis=1)      # per env, by global id
    up = np.stack([-3e-6 + 0 * g, 1e-7 * g], axis=1)
    mk = lambda n, off: _layered(n, A=A, T=T, global_env_offset=off, total_envs=B, field_angle=angles, sightlines={"up": up}, meta_pupil_pixels=NL,
                                 disturbance=DIST)
    whole, halves = mk(B, 0), [mk(33, 0), mk(33, 33)]
    np.testing.assert_array_equal(whole.field_angle, np.concatenate([h.field_angle for h in halves]))
    acts = _actions(torch, T, B, A)
    cat = lambda xs: torch.cat(list(xs), dim=0)
    assert torch.equal(whole.reset()[0], cat(h.reset()[0] for h in halves))
    for t in range(T):
        rw = whole.step(acts[t])
        rh = [h.step(acts[t, off:off + 33].contiguous()) for h, off in zip(halves, (0, 33))]
        for k, x in enumerate(_step_tensors(rw) + _sight(rw[4], "up")):
            assert torch.equal(x, cat((_step_tensors(r) + _sight(r[4], "up"))[k] for r in rh)), f"step {t}, output {k}"
    assert not torch.equal(rw[4]["power"], rw[4]["sightlines"]["up"]["power"])
    for e in [whole] + halves:
        e.close()


def test_state_restore_resumes_bit_identically():
    """checkpoint_harness.resume_case: a fresh env built alike and the env itself after it has moved on (and looked elsewhere) resume the
    uninterrupted run in every output of the env and of its sightline."""
    T = 4
    theta = (2e-6, 3e-6)

    def make():
        return _layered(5, L=3, altitudes=(0.0, 4e3, 1e4), A=6, T=T, field_angle=theta, sightlines={"up": (-4e-6, 1e-6)}, disturbance=DIST)

    def after(env):
        return list(env.sightlines["up"].last.values()) + [env.disturbance.coeff, env.sightlines["up"].env.wavefront_truth()["rms"]]

    def look_elsewhere(env):
        env.set_field_angle((0.0, 0.0))
        env.sightlines["up"].set_angle((1e-6, 1e-6))
        env.step(ch.actions_at(env))

    n = ch.resume_case(make, ch.drive_with(T, after=after), 6, 5, before_restore=look_elsewhere)
    assert n >= 5 * 12
    env, bare = make(), _layered(5, L=3, altitudes=(0.0, 4e3, 1e4), A=6, T=T, field_angle=theta, disturbance=DIST)
    with pytest.raises(ValueError, match="sightlines"):
        bare.set_state(env.get_state())
    with pytest.raises(ValueError, match="sightlines"):
        env.set_state(bare.get_state())
    env.close(), bare.close()


def test_the_entry_point_runs_on_a_side_stream(cycles_per_ms):  # noqa: F811
    """aog_install_layer_sum_sightline behind a delayed producer on a caller's side stream (stream_harness), held bit for bit to a twin on
    the default stream: the shifts' copy and the three kernels are ordered behind the caller's stream."""
    B, A = 5, 6

    def make():
        return _layered(B, A=A, T=5, field_angle=(2e-6, 3e-6), sightlines={"up": (-4e-6, 1e-6)}, disturbance=DIST)

    def script(env, r):
        up = env.sightlines["up"]
        r.call("reset", lambda: (env.reset()[0], up.env._last_obs))
        for t in range(2):
            a = r.input(_acts(B, A, t))
            # (two layers evolve, the generator advances, two fronts get the sum installed and step)
            r.call(f"step{t}", lambda: env.step(a), weight=8)
        up.set_angle((1e-6, -2e-6))       # new shifts: staged and copied on the caller's stream
        a = r.input(_acts(B, A, 2))
        r.call("step after set_angle", lambda: env.step(a), weight=8)
        state = r.call("get_state", lambda: env.get_state(), blocking="get_state")
        a = r.input(_acts(B, A, 3))
        r.call("set_state + step", lambda: (env.set_state(state), env.step(a))[1], blocking="set_state")

    _both(cycles_per_ms, make, script)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_front_usable(layer_sets):
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A = 33, 6
    layers = layer_sets[NL, B][:2]
    front = _static_env(B, N=N, A=A)
    good = _shifts(B, 2)
    assert _install(front, layers, good)[0] == 0
    before = lref.front_store(front).copy()
    coeff = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    assert _upload(front, np.ones((2, int(front.tables.n_ap))))[0] == 0
    outside, nan, ground = good.copy(), good.copy(), np.zeros((1, B, 2))
    outside[1, 7, 0] = MARGIN - 0.5
    nan[0, B - 1, 1] = np.nan
    ground[0, 2, 1] = 0.25
    wide = _static_env(B, N=NL, A=A, params=_meta_params())       # a front larger than the layers
    odd = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, params=_meta_params(N + 5), **_kw(N=N + 5, A=A, T=0))
    valu = _static_env(B, N=N, A=A, kernel="valu")
    for rc_msg, code, word in ((_install(front, layers, outside), -1, "layer 1, env 7 is outside the margin"),
                               (_install(front, layers, nan), -1, "layer 0, env 32 is outside the margin"),
                               (_install(front, layer_sets[N, B][:1], ground), -1, "c = 0"),
                               (_install(wide, layer_sets[N, B][:1], np.zeros((1, B, 2))), -1, "does not match"),
                               (_install(front, [odd], np.zeros((1, B, 2))), -1, "must be even"),
                               (_install(front, layers, good, coeff), -1, "3 terms"),
                               (_install(valu, layers, good, coeff[:, :1].contiguous()), -1, "aog_upload_disturbance_basis"),
                               (_install(front, [layer_sets[NL, 1][0]], good[:1]), -1, "does not match"),
                               (_install(front, [], good), -1, "0 layers"),
                               (_install(valu, layers, good), -4, "VALU")):
        rc, msg = rc_msg
        assert rc == code and word in msg and "aog_install_layer_sum_sightline" in msg, (rc, msg)
    if torch.cuda.device_count() > 1:   # a layer on another device
        far = BatchedAOEnv(B, "cuda:1", atm_type="dynamic", atm_vel=30, atm_fried=0.15, seed=11, params=_meta_params(), **_kw(N=NL, A=A, T=0))
        rc, msg = _install(front, [far], good[:1])
        assert rc == -1 and "does not match" in msg
        far.close()
    # nothing was written; the next valid installation succeeds and the front steps
    np.testing.assert_array_equal(lref.front_store(front), before)
    rc, msg = _install(front, layers, -good, coeff[:, :2].contiguous())
    assert rc == 0, msg
    assert not np.array_equal(lref.front_store(front), before)
    front.reset()
    obs, rew, done, _, info = front.step(_actions(torch, 1, B, A)[0])
    assert bool(torch.isfinite(info["obs_raw"]).all()) and 0 <= float(info["strehl"].min()) <= float(info["strehl"].max()) <= 1
    assert front.device_status() == 0
    for e in (front, wide, odd, valu):
        e.close()
