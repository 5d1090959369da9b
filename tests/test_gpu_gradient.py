"""The analytic gradient of observation, power and Strehl on the device (aog_output_gradient: k_grad_forward / k_grad_coef / k_grad_backward /
k_grad_finish, and the float64 kernels of validation handles) against the numpy restatement tests/gradient_reference.py, which builds the
phase from get_screens(), get_actuators() and env.tables.modes and forms the gradient from the dense per-pixel Jacobian.
Shapes: N = 32 has 812 aperture pixels = 26 pixel tiles with 12 pixels in the last; B = 40 is two env tiles, the second ragged.
Bounds, relative to the largest |gradient| of the row (the largest value for `values`): float64 handles 1e-9 (only the summation order
differs: n_ap eps; measured <= 4e-14); fast handles FAST = 4 x the worst deviation measured at these shapes on the MI355X, 7.6e-6
(profiles/output_gradient.md lists every case), far under the cap 1e-3 above which a bound would stop telling a wrong term from rounding.
Every case prints its worst figure ("WORST ...", run with -s) before it asserts."""
import ctypes as C

import numpy as np
import pytest

import gradient_reference as gr
from helpers import actions_for, assert_short_last_chunk, smooth_screens
from test_gpu_wavefront_truth import CASES, EDGE

pytestmark = pytest.mark.gpu

N, B = 32, 40
FAST, FP64 = 4 * 7.624e-6, 1e-9
assert FAST <= 1e-3
assert_short_last_chunk(EDGE[2])   # N = 52: 67 pixel tiles, the second chunk holds three (a wave without tiles), the last tile 16 pixels
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


def _cotangents(num_envs, n_obs, seed, obs=True):
    """name -> [B, n_obs + 2]: each term alone, so that no missing one can hide, then mixed."""
    rng = np.random.RandomState(seed)
    rows = {}
    if obs and n_obs:
        centre = (int(np.sqrt(n_obs)) // 2) * int(np.sqrt(n_obs)) + int(np.sqrt(n_obs)) // 2
        rows["obs centre"] = np.zeros((num_envs, n_obs + 2))
        rows["obs centre"][:, centre] = 1.0
        rows["obs corner"] = np.zeros((num_envs, n_obs + 2))
        rows["obs corner"][:, 0] = 1.0
    rows["power"] = np.zeros((num_envs, n_obs + 2))
    rows["power"][:, n_obs] = 1.0
    rows["strehl"] = np.zeros((num_envs, n_obs + 2))
    rows["strehl"][:, n_obs + 1] = 1.0
    rows["mix"] = rng.randn(num_envs, n_obs + 2)
    if not (obs and n_obs):
        rows["mix"][:, :n_obs] = 0.0
    return rows


def _split(torch, g, n_obs):
    """a [B, n_obs + 2] cotangent as the three device arguments (a term that is all zero goes in as None)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    go = t(g[:, :n_obs]) if n_obs and np.any(g[:, :n_obs]) else None
    gp = t(g[:, n_obs]) if np.any(g[:, n_obs]) else None
    gs = t(g[:, n_obs + 1]) if np.any(g[:, n_obs + 1]) else None
    return go, gp, gs


def _hold(env, bound, what, seed=1, wrt="actuators", action=None):
    """Every cotangent's gradient, and the values, against the restatement of the env's current state.  Returns the worst deviation."""
    torch = _torch()
    t = env.tables
    sep = env.obs_route == "separable"
    n_obs = env.obs_dim ** 2
    n_ref = 0 if sep else n_obs   # (the reference's rows follow the tables: no observation rows on the separable route)
    scr, act = gr.host_state(env)
    worst = 0.0
    for name, g in _cotangents(env.num_envs, n_obs, seed, obs=not sep).items():
        go, gp, gs = _split(torch, g, n_obs)
        got, values = env.output_gradient(go, gp, gs, wrt=wrt, action=action, with_values=True)
        got, values = got.cpu().numpy(), values.cpu().numpy()
        gref = np.concatenate([g[:, :n_ref], g[:, n_obs:]], axis=1)
        ref = gr.grad_actuators(scr, act, t, gref)
        if wrt == "action":
            ref = gr.chain_to_action(ref, action.cpu().numpy(), t)
        scale = np.abs(ref).max(axis=1)
        assert np.all(scale > 0), f"{what}, {name}: the reference gradient of some env is identically zero: the case checks nothing"
        dev = float(np.max(np.abs(got - ref).max(axis=1) / scale))
        print(f"{what}, {name}: max deviation / largest |gradient| {dev:.2e}   (|gradient| {scale.min():.3e} .. {scale.max():.3e})")
        worst = max(worst, dev)
        assert dev <= bound, f"{what}, {name}: gradient deviates {dev:.3e} > {bound:g}"
    vref = gr.values_of(gr.phase(scr, act, t), t)
    if sep:
        assert np.all(np.isnan(values[:, :n_obs]))
        values = values[:, n_obs:]
    vdev = float(np.max(np.abs(values - vref).max(axis=1) / np.abs(vref).max(axis=1)))
    print(f"{what}: values, max deviation / largest value {vdev:.2e}")
    assert vdev <= bound, f"{what}: values deviate {vdev:.3e} > {bound:g}"
    return max(worst, vdev)


# ---- 1. parity with the restatement --------------------------------------------------------------------------------------------------------
def test_a_shape_exercises_the_pad_pixels():
    _torch()
    env = _env(2)
    try:
        assert env.tables.n_ap % 32 != 0, "no parity shape has a ragged last pixel tile"
    finally:
        env.close()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("o", [2, 5])
@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_parity_with_the_restatement(case, o, precision):
    torch = _torch()
    act_type, A, n = CASES[case]
    bound = FAST if precision == "fast" else FP64
    env = _env(B, act_type, A, n, obs_dim=o, screens=smooth_screens(B, n, 31), precision=precision)
    try:
        env.reset()
        w = _hold(env, bound, f"{case} o={o} {precision} after reset (flat mirror)")
        for t in range(2):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = max(w, _hold(env, bound, f"{case} o={o} {precision} after two steps", seed=2))
        print(f"WORST {case} o={o} {precision}: {w:.3e}")
    finally:
        env.close()


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_parity_where_a_wave_has_no_tile(precision):
    torch = _torch()
    act_type, A, n = EDGE
    bound = FAST if precision == "fast" else FP64
    env = _env(B, act_type, A, n, obs_dim=2, screens=smooth_screens(B, n, 31), precision=precision)
    try:
        env.reset()
        w = _hold(env, bound, f"edge52 o=2 {precision} after reset (flat mirror)")
        for t in range(2):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = max(w, _hold(env, bound, f"edge52 o=2 {precision} after two steps", seed=2))
        print(f"WORST edge52 o=2 {precision}: {w:.3e}")
    finally:
        env.close()


# ---- 2. the action chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_grad_action_parity(precision):
    torch = _torch()
    A = 20
    bound = FAST if precision == "fast" else FP64
    env = _env(B, act_dim=A, screens=smooth_screens(B, N, 32), precision=precision)
    try:
        env.reset()
        a = torch.from_numpy(actions_for(B, A, 7)).cuda()
        env.step(a)
        w = _hold(env, bound, f"grad_action {precision}", seed=3, wrt="action", action=a)
        print(f"WORST grad_action {precision}: {w:.3e}")
        # on the device: the outputs do not change with the action's scale
        g = env.output_gradient(g_strehl=torch.ones(B, dtype=torch.float64, device="cuda:0"), wrt="action")   # (the last step's action)
        assert torch.equal(g, env.output_gradient(g_strehl=torch.ones(B, dtype=torch.float64, device="cuda:0"), wrt="action", action=a))
        a64 = a.to(torch.float64)
        dot, lim = (a64 * g).sum(dim=1).abs(), a64.norm(dim=1) * g.norm(dim=1)
        print(f"grad_action {precision}: |a . grad| / (|a| |grad|) {float((dot / lim).max()):.2e}")
        assert bool((lim > 0).all()) and bool((dot <= bound * lim).all())
    finally:
        env.close()


def test_grad_action_is_refused_on_raw_actuator_handles():
    torch = _torch()
    env = _env(B, act_dim=20, SH_operation=True)
    try:
        env.reset()
        a = torch.zeros((B, 20), dtype=torch.float32, device="cuda:0")
        env.step(a)
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, 20), dtype=torch.float64, device="cuda:0")
        env.output_gradient(g_strehl=one)   # (uploads)
        p = C.c_void_p
        rc = env.lib.aog_output_gradient(env._handle, None, None, p(one.data_ptr()), p(a.data_ptr()), None, p(out.data_ptr()), None, env._stream())
        assert rc == -1 and b"sh_operation" in env.lib.aog_last_error()
    finally:
        env.close()


# ---- 3. dynamic atmosphere -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_dynamic_parity(extrusion):
    torch = _torch()
    A = 20
    env = _env(B, act_dim=A, atm_type="dynamic", atm_vel=20.0, extrusion=extrusion)
    try:
        env.reset()
        for t in range(3):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
        w = _hold(env, FAST, f"dynamic, extrusion={extrusion}, after three steps")
        print(f"WORST dynamic {extrusion}: {w:.3e}")
    finally:
        env.close()


def _blob(torch, env):
    """The library's state blob in a zeroed buffer (its parts start on 256-byte boundaries: the gaps between them are never written)."""
    blob = torch.zeros((int(env.lib.aog_state_bytes(env._handle)),), dtype=torch.uint8, device="cuda:0")
    ts = C.c_int64()
    rc = env.lib.aog_get_state(env._handle, C.c_void_p(blob.data_ptr()), C.byref(ts), env._stream())
    assert rc == 0, env.lib.aog_last_error()
    torch.cuda.synchronize()
    return blob, int(ts.value)


# ---- 4. nothing else moves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(atm_type="quasi_static"), dict(atm_type="dynamic", atm_vel=20.0)], ids=["quasi_static", "dynamic_int8_work_ahead"])
def test_nothing_a_step_reads_or_writes_moves(kw):
    torch = _torch()
    A, T = 20, 4
    env, twin = _env(B, act_dim=A, **kw), _env(B, act_dim=A, **kw)
    try:
        o1, _ = env.reset()
        o2, _ = twin.reset()
        assert torch.equal(o1, o2)
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        for t in range(T):
            g = env.output_gradient(g_power=one, g_strehl=one)   # between every two steps of the episode
            assert bool(torch.isfinite(g).all())
            a = torch.from_numpy(actions_for(B, A, t)).cuda()
            r1, r2 = env.step(a), twin.step(a)
            env.output_gradient(g_obs=torch.ones((B, 4), dtype=torch.float64, device="cuda:0"), wrt="action")
            for k, name in ((0, "obs"), (1, "reward"), (2, "done")):
                assert torch.equal(r1[k], r2[k]), f"step {t}: {name} moved"
            for k in ("power", "strehl", "obs_raw"):
                assert torch.equal(r1[4][k], r2[4][k]), f"step {t}: {k} moved"
            assert torch.equal(env.get_actuators(), twin.get_actuators()), f"step {t}: the mirror moved"
        if env.atm_type == "dynamic":
            assert env.extrusion_kmax > 0   # (the int8 extrusion, whose work ahead the call must leave alone)
        assert torch.equal(env.get_screens(), twin.get_screens())
        (b1, t1), (b2, t2) = _blob(torch, env), _blob(torch, twin)
        assert t1 == t2 and b1.numel() > 0 and torch.equal(b1, b2), "the state blob moved"
        assert env.device_status() == 0
    finally:
        env.close()
        twin.close()


# ---- 5. a split batch reproduces the whole one ----------------------------------------------------------------------------------------------
def test_split_batch_is_bit_identical():
    torch = _torch()
    A = 20
    whole = _env(B, act_dim=A, total_envs=B)
    parts = [_env(32, act_dim=A, global_env_offset=0, total_envs=B), _env(8, act_dim=A, global_env_offset=32, total_envs=B)]
    try:
        a = torch.from_numpy(actions_for(B, A, 3)).cuda()
        g = torch.from_numpy(np.random.RandomState(5).randn(B, 6)).cuda()

        def run(env, sl):
            env.reset()
            env.step(a[sl].contiguous())
            return env.output_gradient(g[sl, :4].contiguous(), g[sl, 4].contiguous(), g[sl, 5].contiguous(), with_values=True)

        ref = run(whole, slice(0, B))
        got = [run(env, sl) for env, sl in zip(parts, (slice(0, 32), slice(32, B)))]
        assert torch.equal(torch.cat([x[0] for x in got]), ref[0]), "grad_act: 32 + 8 envs differ from 40"
        assert torch.equal(torch.cat([x[1] for x in got]), ref[1]), "values: 32 + 8 envs differ from 40"
        assert float(ref[0].abs().max(dim=1).values.min()) > 0
    finally:
        for env in [whole] + parts:
            env.close()


# ---- 6. the separable observation route ----------------------------------------------------------------------------------------------------
def test_separable_route_has_power_and_strehl_gradients():
    torch = _torch()
    A = 20
    env = _env(B, act_dim=A, obs_dim=8, screens=smooth_screens(B, N, 33))
    try:
        assert env.obs_route == "separable"
        env.reset()
        env.step(torch.from_numpy(actions_for(B, A, 1)).cuda())
        w = _hold(env, FAST, "separable o=8")
        print(f"WORST separable: {w:.3e}")
        go = torch.ones((B, 64), dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, A), dtype=torch.float64, device="cuda:0")
        rc = env.lib.aog_output_gradient(env._handle, C.c_void_p(go.data_ptr()), None, None, None, C.c_void_p(out.data_ptr()), None, None, env._stream())
        assert rc == -4 and b"separable" in env.lib.aog_last_error()   # AOG_ERR_UNSUPPORTED
    finally:
        env.close()


# ---- 7. guards -----------------------------------------------------------------------------------------------------------------------------
def test_guards():
    torch = _torch()
    A = 20
    p = C.c_void_p
    env = _env(B, act_dim=A, timesteps_per_episode=3)
    try:
        env.reset()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, A), dtype=torch.float64, device="cuda:0")
        call = lambda cot, res: env.lib.aog_output_gradient(env._handle, None, None, cot, None, res, None, None, env._stream())
        # before the upload
        assert call(p(one.data_ptr()), p(out.data_ptr())) == -3 and b"aog_upload_gradient" in env.lib.aog_last_error()   # AOG_ERR_STATE
        ok = env.output_gradient(g_strehl=one)
        assert call(p(one.data_ptr()), p(out.data_ptr())) == 0 and torch.equal(out, ok)
        assert call(None, p(out.data_ptr())) == -1 and b"cotangent" in env.lib.aog_last_error()   # AOG_ERR_INVALID
        assert call(p(one.data_ptr()), None) == -1 and b"output" in env.lib.aog_last_error()
        # an action pending after a pipelined step
        a = [torch.from_numpy(actions_for(B, A, t)).cuda() for t in range(2)]
        env.step(a[0], next_actions=a[1])
        assert call(p(one.data_ptr()), p(out.data_ptr())) == -3
        with pytest.raises(RuntimeError, match="aog_output_gradient"):
            env.output_gradient(g_strehl=one)
        env.step(a[1], next_actions=None)
        env.output_gradient(g_strehl=one)
        # new tables clear the upload; the binding uploads again
        env.reset()
        env._upload_tables()
        assert call(p(one.data_ptr()), p(out.data_ptr())) == -3 and b"aog_upload_gradient" in env.lib.aog_last_error()
        assert torch.equal(env.output_gradient(g_strehl=one), ok)
    finally:
        env.close()
    # between two steps of a lookahead episode
    env = _env(B, act_dim=A, atm_type="dynamic", atm_vel=20.0, timesteps_per_episode=3)
    try:
        assert env.lookahead(True)
        env.reset()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        env.output_gradient(g_strehl=one)
        for t in range(3):
            env.step(torch.from_numpy(actions_for(B, A, t)).cuda())
            if t < 2:
                with pytest.raises(RuntimeError, match="aog_output_gradient"):
                    env.output_gradient(g_strehl=one)
        env.output_gradient(g_strehl=one)   # the episode's last step never looks ahead
        env.lookahead(False)
    finally:
        env.close()


# ---- 8. it points uphill -------------------------------------------------------------------------------------------------------------------
def test_gradient_ascent_raises_the_strehl():
    """Ten iterations of act += eta grad_act(g_strehl = 1) on static screens, eta from the first gradient so that the first move is 20 nm rms
    of surface.  The condition is that the Strehl rises at every iteration; the distance of the final Strehl to the Marechal value of
    the fitting error, exp(-(2 pi fit_rms / lambda_sci)^2), is printed (profiles/output_gradient.md records it)."""
    torch = _torch()
    A = 20
    env = _env(B, act_dim=A, screens=smooth_screens(B, N, 5, amp=1e-5, sigma_frac=0.15), SH_operation=True)
    try:
        env.reset()
        act = torch.zeros((B, A), dtype=torch.float64, device="cuda:0")
        env.step(act.to(torch.float32))
        fit_rms = env.wavefront_truth()["fit_rms"].cpu().numpy()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        G = torch.from_numpy(np.asarray(env.tables.gram, dtype=np.float64)).cuda()
        g, v = env.output_gradient(g_strehl=one, with_values=True)
        eta = 20e-9 / torch.sqrt(torch.einsum("ei,ij,ej->e", g, G, g))
        strehl = [v[:, -1].clone()]
        for it in range(10):
            act = act + eta[:, None] * g
            env.set_actuators(act)
            env.step(act.to(torch.float32))
            g, v = env.output_gradient(g_strehl=one, with_values=True)
            strehl.append(v[:, -1].clone())
            rise = (strehl[-1] - strehl[-2])
            print(f"iteration {it + 1}: Strehl {float(strehl[-1].min()):.4f} .. {float(strehl[-1].max()):.4f}, smallest rise {float(rise.min()):.3e}")
            assert bool((rise > 0).all()), f"iteration {it + 1}: the Strehl of some env did not rise"
        marechal = np.exp(-(2.0 * np.pi * fit_rms / env.params.wavelength_sci) ** 2)
        margin = marechal - strehl[-1].cpu().numpy()
        print(f"after ten iterations: Marechal value of the fitting error minus the Strehl reached: {margin.min():.3e} .. {margin.max():.3e}")
    finally:
        env.close()


# ---- 9. autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_backward_is_one_gradient_call():
    torch = _torch()
    from adaptive_optics_gym_amd.autograd import step_outputs

    A = 20
    env = _env(B, act_dim=A)
    try:
        env.reset()
        rng = np.random.RandomState(11)
        W = [torch.from_numpy(rng.randn(*s)).cuda() for s in ((B, 4), (B,), (B,))]
        a = torch.from_numpy(actions_for(B, A, 2)).cuda().to(torch.float64).requires_grad_(True)   # (a float64 leaf: its gradient is not rounded)
        obs_raw, power, strehl = step_outputs(env, a)
        assert obs_raw.dtype == torch.float64 and tuple(obs_raw.shape) == (B, 4)
        loss = (obs_raw * W[0]).sum() + (power * W[1]).sum() + (strehl * W[2]).sum()
        loss.backward()
        want = env.output_gradient(W[0], W[1], W[2], wrt="action")
        assert float(want.abs().max()) > 0 and torch.equal(a.grad, want)
        # the state has moved on: the first graph's backward is refused
        b = a.detach().clone().requires_grad_(True)
        out1 = step_outputs(env, b)
        env.step(a.detach().to(torch.float32))
        with pytest.raises(RuntimeError, match="stepped, reset or restored"):
            out1[2].sum().backward()
    finally:
        env.close()
