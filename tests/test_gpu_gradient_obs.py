"""The observation gradient on the separable observation route (aog_upload_gradient_obs; k_grad_obs_field / k_grad_obs_q /
k_grad_obs_backward behind K11's pass 1, and the float64 kernels of validation handles) against the numpy restatement
tests/gradient_obs_reference.py, which builds F from env.tables.obs_m1 / obs_m2 / ap_index and the gradient from the dense per-pixel Jacobian.
Shapes: B = 40 is two env tiles, the second ragged; N = 32 is one x tile of the grid, N = 40 pads x to 64 and y to 48 (both ragged: the
second y tile of the q kernel has 16 rows); o = 6 / 8 fill half a k-step, o = 17 the second k-step in part, o = 32 the whole block.
Cotangents: with c = o // 2 one-hot pixels (c, c) and (c + 1, c - 2) — asymmetric in offset and sign, so a swapped v / u or a conjugate
shows — power alone, Strehl alone, and a random mix over all o^2 + 2 entries.  Corner pixels are left out as one-hots: on these tables
they carry <= 1e-3 of the peak, where the fp32 phases dominate.
Bounds, relative to the largest |gradient| of the row (the largest value for `values`): float64 handles 1e-9 (only the summation order
differs); fast handles FAST = 4 x the worst deviation measured at these shapes on the MI355X (profiles/output_gradient_separable.md lists
every case), under the cap 1e-3.  Every case prints its worst figure ("WORST ...", run with -s) before it asserts."""
import ctypes as C

import numpy as np
import pytest

import gradient_obs_reference as gor
import gradient_reference as gr
from helpers import actions_for, assert_short_last_chunk, smooth_screens
from test_gpu_wavefront_truth import CASES, EDGE

pytestmark = pytest.mark.gpu

B = 40
FAST, FP64 = 4 * 2.629e-6, 1e-9   # (profiles/output_gradient_separable.md: the worst case is apad16, power after reset)
assert FAST <= 1e-3
assert_short_last_chunk(EDGE[2])   # N = 52: 67 pixel tiles, the second chunk holds three (a wave without tiles), the last tile 16 pixels
_TABLES = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _kw(act_type="num_actuators", act_dim=20, n=32, **kw):
    from adaptive_optics_gym_amd.optics_host import build_tables, obs_route_for
    from adaptive_optics_gym_amd.params import OpticalParams

    base = dict(obs_dim=8, timesteps_per_episode=4, seed=17, screen_oversampling=4, verbose=False, obs_gradient=True)
    base.update(kw)
    key = (act_type, act_dim, n, base["obs_dim"], obs_route_for(base.get("precision", "fast"), base["obs_dim"]))
    if key not in _TABLES:   # the host precompute once per shape; every handle of that shape shares it
        _TABLES[key] = build_tables(OpticalParams(num_pupil_pixels=n), act_type, act_dim, base["obs_dim"], obs_route=key[4])
    return dict(act_type=act_type, act_dim=act_dim, num_pupil_pixels=n, tables=_TABLES[key], **base)


def _env(num_envs=B, *a, **kw):
    from adaptive_optics_gym_amd import BatchedAOEnv

    return BatchedAOEnv(num_envs, "cuda:0", **_kw(*a, **kw))


def _cotangents(num_envs, o, seed):
    """name -> [B, o^2 + 2]: each term alone, so that no missing one can hide, then mixed."""
    n_obs, c = o * o, o // 2
    rows = {}
    for name, (v, u) in (("obs (c, c)", (c, c)), ("obs (c + 1, c - 2)", (c + 1, c - 2))):
        rows[name] = np.zeros((num_envs, n_obs + 2))
        rows[name][:, v * o + u] = 1.0
    rows["power"] = np.zeros((num_envs, n_obs + 2))
    rows["power"][:, n_obs] = 1.0
    rows["strehl"] = np.zeros((num_envs, n_obs + 2))
    rows["strehl"][:, n_obs + 1] = 1.0
    rows["mix"] = np.random.RandomState(seed).randn(num_envs, n_obs + 2)
    return rows


def _split(torch, g, n_obs):
    """a [B, n_obs + 2] cotangent as the three device arguments (a term that is all zero goes in as None)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return (t(g[:, :n_obs]) if np.any(g[:, :n_obs]) else None, t(g[:, n_obs]) if np.any(g[:, n_obs]) else None,
            t(g[:, n_obs + 1]) if np.any(g[:, n_obs + 1]) else None)


def _hold(env, bound, what, seed=1, wrt="actuators", action=None):
    """Every cotangent's gradient, and the values, against the restatement of the env's current state.  Returns the worst deviation."""
    torch = _torch()
    t = env.tables
    o = env.obs_dim
    n_obs = o * o
    scr, act = gr.host_state(env)
    rows = _cotangents(env.num_envs, o, seed)
    refs = gor.grad_actuators(scr, act, t, np.stack(list(rows.values())))   # (one Jacobian per env for all the cotangents)
    worst = 0.0
    values = None
    for (name, g), ref in zip(rows.items(), refs):
        got, values = env.output_gradient(*_split(torch, g, n_obs), wrt=wrt, action=action, with_values=True)
        got = got.cpu().numpy()
        if wrt == "action":
            ref = gr.chain_to_action(ref, action.cpu().numpy(), t)
        scale = np.abs(ref).max(axis=1)
        assert np.all(scale > 0), f"{what}, {name}: the reference gradient of some env is identically zero: the case checks nothing"
        dev = float(np.max(np.abs(got - ref).max(axis=1) / scale))
        print(f"{what}, {name}: max deviation / largest |gradient| {dev:.2e}   (|gradient| {scale.min():.3e} .. {scale.max():.3e})")
        worst = max(worst, dev)
        assert dev <= bound, f"{what}, {name}: gradient deviates {dev:.3e} > {bound:g}"
    vref = gor.values_of(gr.phase(scr, act, t), t)
    values = values.cpu().numpy()
    vdev = float(np.max(np.abs(values - vref).max(axis=1) / np.abs(vref).max(axis=1)))
    print(f"{what}: values, max deviation / largest value {vdev:.2e}")
    assert vdev <= bound, f"{what}: values deviate {vdev:.3e} > {bound:g}"
    return max(worst, vdev)


def _parity(what, precision, act_type, A, n, o):
    torch = _torch()
    bound = FAST if precision == "fast" else FP64
    env = _env(B, act_type, A, n, obs_dim=o, screens=smooth_screens(B, n, 31), precision=precision)
    try:
        assert env.obs_route == "separable" and env.obs_gradient
        env.reset()
        w = _hold(env, bound, f"{what} after reset (flat mirror)")
        for t in range(2):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = max(w, _hold(env, bound, f"{what} after two steps", seed=2))
        print(f"WORST {what}: {w:.3e}")
    finally:
        env.close()


# ---- 1. parity with the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,o", [(32, 6), (40, 8), (40, 17), (40, 32), (EDGE[2], 8)])
def test_parity_with_the_restatement(n, o):
    _parity(f"N={n} o={o} fast", "fast", "num_actuators", 20, n, o)


@pytest.mark.parametrize("case", list(CASES))
def test_parity_over_the_padded_mode_counts(case):
    act_type, A, n = CASES[case]
    _parity(f"{case} o=8 fast", "fast", act_type, A, n, 8)


@pytest.mark.parametrize("o", [8, 17])
def test_parity_of_the_float64_handle(o):
    _parity(f"N=40 o={o} fp64", "fp64", "num_actuators", 20, 40, o)


def test_values_are_the_observation_the_step_returned():
    """values[:, :o^2] against the step's own float32 obs_raw (k_obs_pass2), within the rule of DESIGN section 2: 1e-5 relative, elements under
    1e-3 of the peak held to 1e-5 x 1e-3 x peak."""
    torch = _torch()
    A, o = 20, 8
    env = _env(B, "num_actuators", A, 40, obs_dim=o, screens=smooth_screens(B, 40, 34))
    try:
        env.reset()
        r = env.step(torch.from_numpy(actions_for(B, A, 1)).cuda())
        step_raw = r[4]["obs_raw"].to(torch.float64).cpu().numpy()
        _, values = env.output_gradient(g_strehl=torch.ones(B, dtype=torch.float64, device="cuda:0"), wrt=None, with_values=True)
        got = values[:, :o * o].cpu().numpy()
        peak = step_raw.max(axis=1, keepdims=True)
        excess = np.abs(got - step_raw) / (1e-5 * np.maximum(np.abs(step_raw), 1e-3 * peak))
        print(f"WORST values against the step's obs_raw: {excess.max():.3e} of the tolerance")
        assert np.all(peak > 0) and excess.max() <= 1.0
    finally:
        env.close()


# ---- 2. the action chain -------------------------------------------------------------------------------------------------------------------
def test_grad_action_parity():
    torch = _torch()
    A, o = 20, 8
    env = _env(B, "num_actuators", A, 40, obs_dim=o, screens=smooth_screens(B, 40, 32))
    try:
        env.reset()
        a = torch.from_numpy(actions_for(B, A, 7)).cuda()
        env.step(a)
        w = _hold(env, FAST, "grad_action", seed=3, wrt="action", action=a)
        print(f"WORST grad_action: {w:.3e}")
        g = env.output_gradient(g_obs=torch.from_numpy(np.random.RandomState(4).randn(B, o * o)).cuda(), wrt="action")
        a64 = a.to(torch.float64)
        dot, lim = (a64 * g).sum(dim=1).abs(), a64.norm(dim=1) * g.norm(dim=1)
        print(f"grad_action: |a . grad| / (|a| |grad|) {float((dot / lim).max()):.2e}")
        assert bool((lim > 0).all()) and bool((dot <= 1e-12 * lim).all())
    finally:
        env.close()


# ---- 3. dynamic atmosphere, 4. a layered front ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_dynamic_parity(extrusion):
    torch = _torch()
    A = 20
    env = _env(B, "num_actuators", A, 32, obs_dim=8, atm_type="dynamic", atm_vel=20.0, extrusion=extrusion)
    try:
        env.reset()
        for t in range(3):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = _hold(env, FAST, f"dynamic, extrusion={extrusion}, after three steps")
        print(f"WORST dynamic {extrusion}: {w:.3e}")
    finally:
        env.close()


def test_layered_front_parity():
    torch = _torch()
    from adaptive_optics_gym_amd import LayeredAOEnv

    A = 20
    kw = _kw("num_actuators", A, 32, obs_dim=8)
    env = LayeredAOEnv(B, "cuda:0", atm_layers=[{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}], atm_fried=0.15, **kw)
    try:
        assert env.obs_gradient
        env.reset()
        for t in range(2):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = _hold(env, FAST, "layered front, two layers, after two steps")   # (host_state reads get_screens(): the float64 sum)
        print(f"WORST layered: {w:.3e}")
    finally:
        env.close()


# ---- 5. a split batch, and the round size, change no bit ------------------------------------------------------------------------------------
def test_split_batch_and_round_size_are_bit_identical(monkeypatch):
    torch = _torch()
    A, o, n = 20, 8, 32
    a = torch.from_numpy(actions_for(B, A, 3)).cuda()
    g = torch.from_numpy(np.random.RandomState(5).randn(B, o * o + 2)).cuda()

    def run(env, sl):
        try:
            env.reset()
            env.step(a[sl].contiguous())
            return env.output_gradient(g[sl, :o * o].contiguous(), g[sl, o * o].contiguous(), g[sl, o * o + 1].contiguous(), with_values=True)
        finally:
            env.close()

    ref = run(_env(B, "num_actuators", A, n, obs_dim=o, total_envs=B), slice(0, B))
    got = [run(_env(20, "num_actuators", A, n, obs_dim=o, global_env_offset=off, total_envs=B), slice(off, off + 20)) for off in (0, 20)]
    assert torch.equal(torch.cat([x[0] for x in got]), ref[0]), "grad_act: 20 + 20 envs differ from 40"
    assert torch.equal(torch.cat([x[1] for x in got]), ref[1]), "values: 20 + 20 envs differ from 40"
    assert float(ref[0].abs().max(dim=1).values.min()) > 0 and bool(torch.isfinite(ref[1]).all())
    # rounds of one env tile instead of both (AOG_GRAD_OBS_CHUNK is read by aog_upload_gradient_obs)
    monkeypatch.setenv("AOG_GRAD_OBS_CHUNK", "32")
    small = run(_env(B, "num_actuators", A, n, obs_dim=o, total_envs=B), slice(0, B))
    assert torch.equal(small[0], ref[0]) and torch.equal(small[1], ref[1]), "rounds of 32 envs differ from one round of 64"


# ---- 6. nothing else moves -----------------------------------------------------------------------------------------------------------------
def _blob(torch, env):
    blob = torch.zeros((int(env.lib.aog_state_bytes(env._handle)),), dtype=torch.uint8, device="cuda:0")
    ts = C.c_int64()
    rc = env.lib.aog_get_state(env._handle, C.c_void_p(blob.data_ptr()), C.byref(ts), env._stream())
    assert rc == 0, env.lib.aog_last_error()
    torch.cuda.synchronize()
    return blob, int(ts.value)


@pytest.mark.parametrize("mode", ["detector", "pipelined"])
def test_nothing_a_step_reads_or_writes_moves(mode):
    torch = _torch()
    A, o, T = 20, 8, 4
    kw = dict(obs_photons=1e4, obs_read_noise=2.0) if mode == "detector" else {}
    env, twin = _env(B, "num_actuators", A, 32, obs_dim=o, **kw), _env(B, "num_actuators", A, 32, obs_dim=o, obs_gradient=False, **kw)
    try:
        o1, _ = env.reset()
        o2, _ = twin.reset()
        assert torch.equal(o1, o2)
        go = torch.from_numpy(np.random.RandomState(6).randn(B, o * o)).cuda()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        acts = [torch.from_numpy(actions_for(B, A, t)).cuda() for t in range(T)]
        for t in range(T):
            # pipelined: steps in pairs (while an action is pending the call is refused, as on every handle): calls between the pairs
            nxt = dict(next_actions=acts[t + 1] if t % 2 == 0 else None) if mode == "pipelined" else {}
            if not (mode == "pipelined" and t % 2 == 1):
                g = env.output_gradient(g_obs=go, g_power=one)
                assert bool(torch.isfinite(g).all())
            r1, r2 = env.step(acts[t], **nxt), twin.step(acts[t], **nxt)
            if not (mode == "pipelined" and t % 2 == 0):
                env.output_gradient(g_obs=go, wrt="action", action=acts[t], with_values=True)
            for k, name in ((0, "obs"), (1, "reward"), (2, "done")):
                assert torch.equal(r1[k], r2[k]), f"step {t}: {name} moved"
            for k in ("power", "strehl", "obs_raw"):
                assert torch.equal(r1[4][k], r2[4][k]), f"step {t}: {k} moved"
            if not (mode == "pipelined" and t % 2 == 0):   # (the mirror cannot be read while an action is pending)
                assert torch.equal(env.get_actuators(), twin.get_actuators()), f"step {t}: the mirror moved"
        assert torch.equal(env.get_screens(), twin.get_screens())
        (b1, t1), (b2, t2) = _blob(torch, env), _blob(torch, twin)
        assert t1 == t2 and b1.numel() > 0 and torch.equal(b1, b2), "the state blob moved"
        assert env.device_status() == 0
    finally:
        env.close()
        twin.close()


# ---- 7. without g_obs the upload changes nothing but the observation slots of values ----------------------------------------------------------
def test_without_g_obs_the_upload_changes_no_bit():
    torch = _torch()
    A, o = 20, 8
    env, twin = _env(B, "num_actuators", A, 32, obs_dim=o), _env(B, "num_actuators", A, 32, obs_dim=o, obs_gradient=False)
    try:
        assert env.obs_gradient and not twin.obs_gradient
        a = torch.from_numpy(actions_for(B, A, 2)).cuda()
        gp, gs = (torch.from_numpy(np.random.RandomState(7 + i).randn(B)).cuda() for i in range(2))
        for e in (env, twin):
            e.reset()
            e.step(a)
        for wrt in ("actuators", "action"):
            (g1, v1), (g2, v2) = (e.output_gradient(None, gp, gs, wrt=wrt, action=a, with_values=True) for e in (env, twin))
            assert float(g2.abs().max()) > 0 and torch.equal(g1, g2), f"wrt={wrt}: the gradient moved"
            assert torch.equal(v1[:, o * o:], v2[:, o * o:])
            assert bool(torch.isnan(v2[:, :o * o]).all()) and bool(torch.isfinite(v1[:, :o * o]).all()) and float(v1[:, :o * o].min()) >= 0
        assert torch.equal(env.output_gradient(None, gp, gs), twin.output_gradient(None, gp, gs))   # (without values)
        go = torch.ones((B, o * o), dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, A), dtype=torch.float64, device="cuda:0")
        rc = twin.lib.aog_output_gradient(twin._handle, C.c_void_p(go.data_ptr()), None, None, None, C.c_void_p(out.data_ptr()), None, None, twin._stream())
        assert rc == -4 and b"separable" in twin.lib.aog_last_error()   # AOG_ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="obs_gradient"):
            _env(2, "num_actuators", A, 32, obs_dim=2)   # (a table-route env has the gradient already)
    finally:
        env.close()
        twin.close()


# ---- 8. guards -----------------------------------------------------------------------------------------------------------------------------
def test_upload_guards():
    torch = _torch()
    A = 20
    env, tab = _env(B, "num_actuators", A, 32, obs_dim=8), _env(B, "num_actuators", A, 32, obs_dim=2, obs_gradient=False)
    lib = env.lib
    try:
        mft = C.byref(env._obs_mft_keep[2])
        up = lambda h: lib.aog_upload_gradient_obs(h, mft)
        # a table-route handle
        assert up(tab._handle) == -3 and b"aog_upload_gradient_obs" in lib.aog_last_error() and b"obs_separable" in lib.aog_last_error()
        # before aog_upload_gradient (the binding uploads both lazily, on the first output_gradient)
        assert up(env._handle) == -3 and b"aog_upload_gradient_obs before aog_upload_gradient" in lib.aog_last_error()
        env.reset()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        go = torch.ones((B, 64), dtype=torch.float64, device="cuda:0")
        ok = env.output_gradient(g_obs=go, g_strehl=one)
        assert up(env._handle) == 0   # (again: the tables are rewritten in place)
        assert torch.equal(env.output_gradient(g_obs=go, g_strehl=one), ok)
        bad = _C_mft(env, 7)
        assert lib.aog_upload_gradient_obs(env._handle, C.byref(bad)) == -1 and b"aog_upload_gradient_obs: o = 7" in lib.aog_last_error()
        # a fresh aog_upload_tables clears both uploads; the binding uploads again
        assert lib.aog_upload_tables(env._handle, C.byref(env._upload_keep[1])) == 0, lib.aog_last_error()
        env._gradient_uploaded = False   # (what BatchedAOEnv._upload_tables notes)
        assert up(env._handle) == -3 and b"aog_upload_gradient_obs before aog_upload_gradient" in lib.aog_last_error()
        out = torch.empty((B, A), dtype=torch.float64, device="cuda:0")
        p = C.c_void_p
        assert lib.aog_output_gradient(env._handle, p(go.data_ptr()), None, None, None, p(out.data_ptr()), None, None, env._stream()) == -3
        assert torch.equal(env.output_gradient(g_obs=go, g_strehl=one), ok)
        # a bare separable handle: before aog_upload_tables, then before aog_upload_obs_mft
        full = env._handle
        env._create_handle("fast", "auto", 0)
        bare, env._handle = env._handle, full
        try:
            assert up(bare) == -3 and b"aog_upload_gradient_obs before aog_upload_tables" in lib.aog_last_error()
            assert lib.aog_upload_tables(bare, C.byref(env._upload_keep[1])) == 0, lib.aog_last_error()
            assert up(bare) == -3 and b"aog_upload_gradient_obs before aog_upload_obs_mft" in lib.aog_last_error()
        finally:
            lib.aog_destroy(bare)
    finally:
        env.close()
        tab.close()


def _C_mft(env, o):
    from adaptive_optics_gym_amd import _lib

    keep = env._obs_mft_keep
    return _lib.AogObsMft(o, 0, keep[2].m1, keep[2].m2)


# ---- 9. autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_differentiates_through_the_observation():
    torch = _torch()
    from adaptive_optics_gym_amd.autograd import step_outputs

    A, o = 20, 8
    env = _env(B, "num_actuators", A, 32, obs_dim=o)
    try:
        env.reset()
        W = torch.from_numpy(np.random.RandomState(11).randn(B, o * o)).cuda()
        a = torch.from_numpy(actions_for(B, A, 2)).cuda().to(torch.float64).requires_grad_(True)   # (a float64 leaf: its gradient is not rounded)
        obs_raw, power, strehl = step_outputs(env, a)
        assert obs_raw.dtype == torch.float64 and tuple(obs_raw.shape) == (B, o * o) and bool(torch.isfinite(obs_raw).all())
        loss = (obs_raw * W).sum() + (obs_raw[:, o * (o // 2) + o // 2] * power).sum()   # a torch-written loss on the image
        loss.backward()
        g_obs = W.clone()
        g_obs[:, o * (o // 2) + o // 2] += power.detach()
        want = env.output_gradient(g_obs, obs_raw.detach()[:, o * (o // 2) + o // 2].contiguous(), torch.zeros_like(power), wrt="action")
        assert float(want.abs().max()) > 0 and torch.equal(a.grad, want)
    finally:
        env.close()
