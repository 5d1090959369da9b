"""aog_pyramid_gradient on the device (fast and float64 handles) against the host restatement in pyramid_gradient_reference.py: the gradient over the
sensor's launch geometries and kinds of cotangent, the returned clean values, what the call must leave alone, independence of how envs are
grouped, ``autograd.pyramid_slopes`` and the refusals."""
import ctypes as C

import numpy as np
import pytest

import pyramid_gradient_reference as gref
import pyramid_reference as ref
from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

# Worst |gradient - restatement| / (the row's largest |gradient|) measured over CONFIGS x the three kinds of call on an MI355X
# (profiles/pyramid_gradient.md), and the bound held: 4 x, the convention of test_gpu_gradient_obs.py.
FP64_WORST, FAST_WORST = 1.9e-14, 1.52e-6
BOUND = {"fp64": 4 * FP64_WORST, "fast": 4 * FAST_WORST}

# (N, A, w_q, n_s, n_mod, r_mod), B = 33 (one full env tile and a pad tile holding one env): the smallest window; a quadrant that is no
# multiple of 16; w = 64 with a detector of two 32-blocks at N = 64
B = 33
CONFIGS = [(32, 20, 8, 8, 1, 0.0), (32, 20, 12, 8, 3, 1.0), (64, 20, 32, 40, 2, 2.0)]
IDS = ["N%d-A%d-wq%d-ns%d-mod%d" % c[:5] for c in CONFIGS]
KW = dict(obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=5, verbose=False)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _sensor_kw(c):
    return dict(samples=c[2], pixels=c[3], n_mod=c[4], r_mod=c[5])


def _make(c, n=B, offset=0, precision="fp64", photons=None, seed=11):
    """An env of config c on envs [offset, offset + n) of the B screens, reset and stepped once (non-zero actuators)."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    N, A = c[:2]
    scr = smooth_screens(B, N, 70 + N, amp=1e-5)
    a = actions_for(B, A, 4)
    sensor = dict(_sensor_kw(c), photons=photons)
    env = BatchedAOEnv(n, "cuda:0", act_type="num_actuators", act_dim=A, num_pupil_pixels=N, screens=scr[offset:offset + n], precision=precision,
                       global_env_offset=offset, total_envs=B, seed=seed, pyramid=sensor, **KW)
    env.reset()
    env.step(torch.from_numpy(a[offset:offset + n]).cuda())
    return env, scr


def _cotangents(c, n_valid):
    """The three calls' cotangents, a different one per env: (g_frames [B, 4, n_s, n_s] | None, g_slopes [B, 2 n_valid] | None) each."""
    ns = c[3]
    rng = np.random.default_rng(17)
    # one-hot frame pixels at a centre and at an edge of each quadrant, then a dense random frame
    gf = np.zeros((B, 4, ns, ns))
    for b in range(B):
        kind = b % 9
        if kind == 8:
            gf[b] = rng.standard_normal((4, ns, ns))
        else:
            gf[b, kind // 2, (ns // 2, 0)[kind % 2], ns // 2] = 1.0 + 0.5 * b
    # one-hot slopes (first s_x, last s_y, a middle s_x), then a dense random vector
    gs = np.zeros((B, 2 * n_valid))
    for b in range(B):
        kind = b % 4
        if kind == 3:
            gs[b] = rng.standard_normal(2 * n_valid)
        else:
            gs[b, (0, 2 * n_valid - 1, n_valid // 2)[kind]] = -1.0 - 0.25 * b
    return [(gf, None), (None, gs), (rng.standard_normal(gf.shape), rng.standard_normal(gs.shape))]


@pytest.mark.parametrize("precision", ["fast", "fp64"])
@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_handle_matches_the_restatement(c, precision):
    """Every env of the batch, every kind of cotangent (one-hot frame pixels at a centre and an edge of each quadrant, one-hot slopes, dense
    random ones, both at once), against pyramid_gradient_reference.grad.  Measured worst error as a fraction of the row's largest
    |gradient| on an MI355X for the three configurations: float64 handles 3.9e-15, 2.8e-15, 1.9e-14; fast handles 1.2e-6, 1.1e-6, 1.5e-6
    (profiles/pyramid_gradient.md); held: 4 x the worst of each precision."""
    torch = _torch()
    env, scr = _make(c, precision=precision)
    act = env.get_actuators().cpu().numpy()
    sensor = ref.Sensor(c[0], env.tables.ap_index, **_sensor_kw(c))
    assert np.array_equal(np.asarray(env._pyramid.valid), sensor.valid)
    worst = 0.0
    for gf, gs in _cotangents(c, sensor.valid.size):
        t = lambda x: None if x is None else torch.from_numpy(x).cuda()
        got = env.pyramid_gradient(g_frames=t(gf), g_slopes=t(gs)).cpu().numpy()
        assert got.shape == (B, c[1]) and got.dtype == np.float64
        for b in range(B):
            want, _, _ = gref.grad(sensor, scr[b], env.tables.modes, act[b], env.wavelength_wfs, None if gf is None else gf[b],
                                   None if gs is None else gs[b])
            assert np.abs(want).max() > 0
            worst = max(worst, float(np.abs(got[b] - want).max() / np.abs(want).max()))
    env.close()
    print(f"pyramid gradient {precision} {c}: worst error {worst:.3e} of the row's largest |gradient|")
    assert worst <= BOUND[precision], f"{worst:.3e} > {BOUND[precision]:.3e}"


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_returned_values_are_the_sensor_calls_bits(precision):
    """frames / slopes of a gradient call at ``actuators=`` equal pyramid_frames / pyramid_slopes of a twin whose mirror stands there, bit
    for bit (the gradient call runs the sensor call's own forward launches), and the mirror of the first env has not moved."""
    torch = _torch()
    c = CONFIGS[1]
    env, _ = _make(c, precision=precision)
    twin, _ = _make(c, precision=precision)
    a0 = env.get_actuators().clone()
    a1 = a0 * 0.7 + 1e-8
    twin.set_actuators(a1.cpu().numpy())
    nv = env._pyramid.n_valid
    g = torch.ones((B, 2 * nv), dtype=torch.float64, device="cuda:0")
    _, frames, slopes = env.pyramid_gradient(g_slopes=g, actuators=a1, with_values=True)
    assert torch.equal(frames, twin.pyramid_frames()) and torch.equal(slopes, twin.pyramid_slopes())
    assert float(frames.max()) > 0 and torch.equal(env.get_actuators(), a0)
    # and at the mirror's own actuators, with a frames cotangent alone
    _, frames, slopes = env.pyramid_gradient(g_frames=torch.ones_like(frames), with_values=True)
    assert torch.equal(frames, env.pyramid_frames()) and torch.equal(slopes, env.pyramid_slopes())
    env.close()
    twin.close()


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_the_call_draws_nothing_and_moves_nothing(precision):
    """With photon noise on, the next pyramid_frames() after a gradient call equals that of a twin that made none (the frame counter of the
    photon stream was not advanced), and the gradient itself is that of the photon-free sensor."""
    torch = _torch()
    c = CONFIGS[0]
    env, _ = _make(c, photons=200.0, precision=precision)
    twin, _ = _make(c, photons=200.0, precision=precision)
    clean, _ = _make(c, precision=precision)
    nv = env._pyramid.n_valid
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((B, 2 * nv))).cuda()
    count = env.pyramid_frame_count
    grad = env.pyramid_gradient(g_slopes=g, actuators=env.get_actuators() * 0.5)
    grad2 = env.pyramid_gradient(g_slopes=g)
    assert env.pyramid_frame_count == count
    assert torch.equal(grad2, clean.pyramid_gradient(g_slopes=g)) and not torch.equal(grad, grad2)
    assert torch.equal(env.get_actuators(), twin.get_actuators())
    f_env, f_twin = env.pyramid_frames(), twin.pyramid_frames()
    assert torch.equal(f_env, f_twin) and not torch.equal(f_env, clean.pyramid_frames())
    for e in (env, twin, clean):
        e.close()


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_grouping_masks_and_chunks_change_no_bit(monkeypatch, precision):
    """Two handles of 16 + 17 envs, a mask and AOG_PYRAMID_CHUNK=1 reproduce the 33-env result bit for bit; masked-out rows keep a sentinel."""
    torch = _torch()
    c = CONFIGS[1]
    rng = np.random.default_rng(9)
    ns = c[3]

    def run(n, offset, chunk=None, mask=None):
        if chunk:
            monkeypatch.setenv("AOG_PYRAMID_CHUNK", str(chunk))
        else:
            monkeypatch.delenv("AOG_PYRAMID_CHUNK", raising=False)
        env, _ = _make(c, n=n, offset=offset, precision=precision)
        nv = env._pyramid.n_valid
        r = np.random.default_rng(9)
        gf = torch.from_numpy(r.standard_normal((B, 4, ns, ns))[offset:offset + n]).cuda()
        gs = torch.from_numpy(r.standard_normal((B, 2 * nv))[offset:offset + n]).cuda()
        env.pyramid_gradient(g_frames=gf, g_slopes=gs)   # (allocates; uploads what a fast handle needs)
        res = (torch.full((n, c[1]), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((n, 4, ns, ns), 7.0, dtype=torch.float64, device="cuda:0"),
               torch.full((n, 2 * nv), 7.0, dtype=torch.float64, device="cuda:0"))
        m = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        assert env.lib.aog_pyramid_gradient(env._handle, p(m), p(gf), p(gs), None, p(res[0]), p(res[1]), p(res[2]), env._stream()) == 0
        torch.cuda.synchronize()
        env.close()
        return res

    whole = run(B, 0)
    assert float(whole[0].abs().max()) > 0
    halves = [run(16, 0), run(17, 16)]
    for k in range(3):
        assert torch.equal(torch.cat([halves[0][k], halves[1][k]]), whole[k])
    chunked = run(B, 0, chunk=1)
    assert all(torch.equal(chunked[k], whole[k]) for k in range(3))
    sel = rng.random(B) < 0.5
    sel[[0, B - 1]] = True, False
    masked = run(B, 0, mask=sel)
    keep = torch.from_numpy(sel).cuda()
    for k in range(3):
        assert torch.equal(masked[k][keep], whole[k][keep])
    assert all(bool((masked[k][~keep] == 7.0).all()) for k in range(3))


@pytest.mark.parametrize("precision", ["fast", "fp64"])
def test_autograd_pyramid_slopes_directional_derivative(precision):
    """d/dt of L = 1/2 |s(a + t d) - s0|^2 at t = 0 from autograd.pyramid_slopes' backward against a central difference of the device's
    loss.  The difference quotient is taken on a float64 handle (step 1e-6 of a wave: truncation and rounding both below 1e-9, as the host
    test of the restatement finds), with the slopes target s0 of the handle under test: on a fast handle the sensor's own fp32 rounding
    (5.9e-7 of the frame peak) over any usable step is 3e-5 of |grad| |d| (measured), five times the tolerance, so its own loss cannot
    referee its gradient.  Held: 1e-6 of |grad| |d| on the float64 handle (measured 2.9e-11), the fast-handle tolerance above on the fast one."""
    torch = _torch()
    from adaptive_optics_gym_amd import autograd

    c = CONFIGS[1]
    env, _ = _make(c, precision=precision)
    ref_env = env if precision == "fp64" else _make(c, precision="fp64")[0]
    lam = env.wavelength_wfs
    a0 = env.get_actuators().clone()
    s0 = env.pyramid_slopes().clone()          # the slopes at the mirror's own actuators: the target
    a = (a0 * 0.6).requires_grad_(True)
    loss = 0.5 * ((autograd.pyramid_slopes(env, a) - s0) ** 2).sum(dim=1)
    (grad,) = torch.autograd.grad(loss.sum(), a)
    assert grad.shape == a.shape and grad.dtype == torch.float64
    d = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(a.shape))).cuda()
    h = 1e-6 * lam / float(np.abs(env.tables.modes).max()) / float(d.abs().max())

    def L(x):
        with torch.no_grad():
            return 0.5 * ((autograd.pyramid_slopes(ref_env, x) - s0) ** 2).sum(dim=1)

    fd = (L(a.detach() + h * d) - L(a.detach() - h * d)) / (2 * h)
    an = (grad * d).sum(dim=1)
    scale = grad.norm(dim=1) * d.norm(dim=1)
    err = float(((fd - an).abs() / scale).max())
    print(f"autograd.pyramid_slopes {precision}: worst |central difference - analytic| {err:.3e} of |grad| |d|; |analytic| / scale up to {float((an.abs() / scale).max()):.3f}")
    assert float(loss.detach().min()) > 0 and err <= (1e-6 if precision == "fp64" else BOUND["fast"])
    if ref_env is not env:
        ref_env.close()
    # the frames function, on the same footing: the gradient of sum(frame) is pyramid_gradient's with a cotangent of ones
    a2 = (a0 * 0.6).requires_grad_(True)
    fr = autograd.pyramid_frames(env, a2)
    (g2,) = torch.autograd.grad(fr.sum(), a2)
    assert torch.equal(g2, env.pyramid_gradient(g_frames=torch.ones_like(fr), actuators=a2.detach()))
    assert torch.equal(fr.detach(), env.pyramid_clean(actuators=a2.detach())[0])
    # the state moves on: backward refuses
    a3 = a0.clone().requires_grad_(True)
    out = autograd.pyramid_slopes(env, a3).sum()
    env.reset()
    with pytest.raises(RuntimeError, match="stepped, reset or restored"):
        out.backward()
    env.close()


def test_refusals():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, _lib

    n, N, A = 5, 32, 16
    kw = dict(act_dim=A, num_pupil_pixels=N, screens=smooth_screens(n, N, 2), **KW)
    grad = torch.zeros((n, A), dtype=torch.float64, device="cuda:0")
    cot = torch.ones(n * 4 * 64 * 64, dtype=torch.float64, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    # before aog_upload_pyramid
    plain = BatchedAOEnv(n, "cuda:0", precision="fp64", **kw)
    base = plain.device_bytes()
    with pytest.raises(ValueError, match="pyramid sensor"):
        plain.pyramid_gradient(g_slopes=cot[:n])
    assert plain.lib.aog_pyramid_gradient(plain._handle, None, p(cot), None, None, p(grad), None, None, None) == -3
    assert b"not uploaded" in plain.lib.aog_last_error() and plain.device_bytes() == base
    plain.close()
    # both cotangents null; no output; a pending pipelined action
    env = BatchedAOEnv(n, "cuda:0", precision="fp64", pyramid=dict(samples=8, pixels=8, n_mod=1, r_mod=0.0), **kw)
    env.reset()
    before = env.device_bytes()
    assert env.lib.aog_pyramid_gradient(env._handle, None, None, None, None, p(grad), None, None, None) == -1 and b"cotangent" in env.lib.aog_last_error()
    assert env.lib.aog_pyramid_gradient(env._handle, None, p(cot), None, None, None, None, None, None) == -1
    acts = torch.from_numpy(np.random.RandomState(6).randn(2, n, A).astype(np.float32)).cuda()
    env.step(acts[0], next_actions=acts[1])   # mid-sequence: the mirror already belongs to the next step
    g = torch.ones((n, 2 * env._pyramid.n_valid), dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.AogError, match="libaogym error -3"):
        env.pyramid_gradient(g_slopes=g)
    env.step(acts[1], next_actions=None)
    assert env.device_bytes() == before       # nothing was allocated by the refused calls
    assert float(env.pyramid_gradient(g_slopes=g).abs().max()) > 0 and env.device_bytes() > before
    env.close()
    # fast handles: built for w_q <= 32; a wider window is refused with the sizes named
    wide = BatchedAOEnv(n, "cuda:0", pyramid=dict(samples=40, pixels=8, n_mod=1, r_mod=0.0), **kw)
    wide.reset()
    with pytest.raises(_lib.AogError, match="libaogym error -4"):
        wide.pyramid_gradient(g_slopes=torch.ones((n, 2 * wide._pyramid.n_valid), dtype=torch.float64, device="cuda:0"))
    assert b"w_q = 40" in wide.lib.aog_last_error()
    assert float(wide.pyramid_clean()[0].max()) > 0
    wide.close()
