"""aog_sh_gradient on the device against the host restatement in shack_gradient_reference.py: the gradient over every launch geometry of the
backward passes and both hipFFT transforms, the returned clean values, what the call must leave alone, ``actuators=``, independence of how
envs are grouped and of the stream, ``autograd.sh_slopes`` and the refusals."""
import ctypes as C

import numpy as np
import pytest

import shack_gradient_reference as sref
from helpers import smooth_screens
from test_gpu_streams import _both, cycles_per_ms  # noqa: F401  (cycles_per_ms: the module's calibration fixture)

pytestmark = pytest.mark.gpu

# Worst |gradient - restatement| / (the row's largest |gradient|) measured over MATRIX x the three kinds of call on an MI355X
# (profiles/shack_gradient.md), per class of handle, and the bound held: 4 x, the convention of test_gpu_pyramid_gradient.py.
# Per case: N128-rl4 3.2e-5, N256-rl8 5.9e-5, N512-rl16-ldshx 8.3e-6, N240-lw60-rl8 2.3e-5, N480-lw60-rl16 2.1e-5, N96-c2c 5.7e-5,
# N128-threepass-c2c 2.3e-5 (complex64: hand-written passes and hipFFT C2C alike); N128-z2z 1.4e-6 (complex128 transforms behind the fast
# handle's fp32 phase).
FP64_WORST, FAST_WORST = 1.444e-6, 5.877e-5
BOUND = {"double": 4 * FP64_WORST, "fast": 4 * FAST_WORST}

A = 8
# id -> (N, B, handle class, constructor keywords, AOG_SH_THREE_PASS): every template instance of the backward passes (RL, LW), the LDS hx
# variant (N = 512), hipFFT C2C and Z2Z, and the generic route on a pruned handle.  B = 33: one full env tile and a pad tile holding one env.
MATRIX = {
    "N128-rl4": (128, 33, "fast", {}, False), "N256-rl8": (256, 5, "fast", {}, False), "N512-rl16-ldshx": (512, 2, "fast", {}, False),
    "N240-lw60-rl8": (240, 5, "fast", {}, False), "N480-lw60-rl16": (480, 2, "fast", {}, False), "N96-c2c": (96, 33, "fast", {}, False),
    "N128-z2z": (128, 33, "double", dict(sh_fft_precision="double"), False), "N128-threepass-c2c": (128, 33, "fast", {}, True),
}
KW = dict(act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=5, SH_operation=True, verbose=False)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _make(key, monkeypatch, n=None, offset=0, seed=11, **extra):
    """(env, screens, actuators of the sensor mirror [n, A]) of MATRIX[key] on envs [offset, offset + n) of its B screens, reset and one
    SH_step taken (the sensor mirror's actuators are non-zero)."""
    from adaptive_optics_gym_amd import BatchedAOEnv

    N, B, _, kw, three = MATRIX[key]
    n = B if n is None else n
    if three:
        monkeypatch.setenv("AOG_SH_THREE_PASS", "1")
    else:
        monkeypatch.delenv("AOG_SH_THREE_PASS", raising=False)
    scr = smooth_screens(B, N, 40 + N, amp=1e-5)
    env = BatchedAOEnv(n, "cuda:0", num_pupil_pixels=N, screens=scr[offset:offset + n], global_env_offset=offset, total_envs=B, seed=seed,
                       **{**KW, **kw, **extra})
    env.reset()
    act, _ = env.SH_step()
    return env, scr[offset:offset + n], act.clone()


def _point(env, screen, act):
    return sref.Point(env.sh, sref.atmosphere_phase(env.sh, screen, env.wavelength_wfs), act, env.sh.amp_wfs, env.params.delta_t)


def _cotangents(env, points):
    """The three calls' (g_image [B, N*N] | None, g_slopes [B, 2 n_sub] | None), a different cotangent per env."""
    sh, B = env.sh, len(points)
    ns, N = sh.n_sub, sh.N
    rng = np.random.default_rng(17)
    gs = np.zeros((B, 2 * ns))
    gi = np.zeros((B, N * N))
    slot2d = sh.sub_slot.reshape(N, N)
    border = np.flatnonzero(((slot2d[:, :-1] >= 0) & (slot2d[:, 1:] >= 0) & (slot2d[:, :-1] != slot2d[:, 1:])).ravel())
    border = (border // (N - 1)) * N + border % (N - 1)          # index in the [N, N] grid of the pixel left of a lenslet border
    for b, p in enumerate(points):
        gs[b, (0, 2 * ns - 1, ns // 2)[b % 3]] = -1.0 - 0.25 * b      # first s_x, last s_y, a middle one
        inside = np.where(sh.sub_slot == (ns // 2 + b) % ns, p.image, -1.0)
        outside = np.where(sh.sub_slot < 0, p.image, -1.0)
        pix = (int(np.argmax(inside)), int(border[(7 * b) % border.size]), int(np.argmax(outside)))[b % 3]
        gi[b, pix] = 1.0 + 0.5 * b                                    # a lenslet's brightest pixel, a border pixel, one outside the selection
    peak = max(float(p.image.max()) for p in points)
    return [(None, gs), (gi, None), (rng.standard_normal(gi.shape) / peak, rng.standard_normal(gs.shape))]


@pytest.mark.parametrize("key", list(MATRIX))
def test_gradient_matches_the_restatement(key, monkeypatch):
    """Every env, three kinds of call (one-hot slopes, one-hot image pixels, a dense mix of both) against shack_gradient_reference.  Measured
    worst error as a fraction of the row's largest |gradient| on an MI355X: see FP64_WORST / FAST_WORST and profiles/shack_gradient.md."""
    torch = _torch()
    env, scr, act = _make(key, monkeypatch)
    B, cls = env.num_envs, MATRIX[key][2]
    a = act.cpu().numpy()
    points = [_point(env, scr[b], a[b]) for b in range(B)]
    worst = 0.0
    for gi, gs in _cotangents(env, points):
        t = lambda x: None if x is None else torch.from_numpy(x).cuda()
        got = env.sh_gradient(g_image=t(gi), g_slopes=t(gs)).cpu().numpy()
        assert got.shape == (B, A) and got.dtype == np.float64
        for b in range(B):
            want = points[b].vjp(None if gi is None else gi[b], None if gs is None else gs[b])
            assert np.abs(want).max() > 0
            worst = max(worst, float(np.abs(got[b] - want).max() / np.abs(want).max()))
    env.close()
    print(f"shack gradient {key} ({cls}): worst error {worst:.3e} of the row's largest |gradient|")
    assert worst <= BOUND[cls], f"{worst:.3e} > {BOUND[cls]:.3e}"


@pytest.mark.parametrize("key", ["N128-rl4", "N240-lw60-rl8", "N96-c2c", "N128-z2z"])
def test_clean_values(key, monkeypatch):
    """sh_clean()'s image is sh_image()'s bit for bit (same route, same launches); the slopes are the restatement's within what the forward's
    image tolerance (5e-6 of the peak in complex64, test_gpu_parity.py; 1e-5 relative in complex128) does to a centroid:
    sum |dI| |x - c| / F per lenslet."""
    env, scr, act = _make(key, monkeypatch)
    image, slopes = env.sh_clean()
    assert image.equal(env.sh_image()) and float(image.max()) > 0
    a = act.cpu().numpy()
    s = slopes.cpu().numpy()
    for b in range(0, env.num_envs, 8):
        p = _point(env, scr[b], a[b])
        dI = 5e-6 * p.image.max() if MATRIX[key][2] == "fast" else 1e-5 * p.image[p.sel]
        tol = np.concatenate([np.bincount(p.slot, weights=dI * np.abs(c), minlength=env.sh.n_sub) / p.flux
                              for c in (p.xs - p.cx[p.slot], p.ys - p.cy[p.slot])])
        assert np.all(np.abs(s[b] - p.slopes) <= tol), float(np.max(np.abs(s[b] - p.slopes) / tol))
    env.close()


def _flat(torch, x):
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        x = list(x.values())
    return [t for v in x for t in _flat(torch, v)] if isinstance(x, (tuple, list)) else []


def _same_actions(torch, a, b, exact):
    """Integrator outputs of two handles.  The estimator fused into the separable route's last pass gives the same bits on every run.
    k_sh_estimate on its own (sh_update, and SH_step of the hipFFT route) sums each lenslet with float64 LDS atomics in whatever order the
    waves arrive: two untouched twins differ in the last bits (measured 1.5e-20 on actuators of 1e-8; test_gpu_parity.py says the same of
    it), so there the comparison is to 1e-12 of the largest actuator, n_pix x 2^-53 of rounding.  A call that touched the noise counter,
    the image or the integrator would move the actuators by 1e-3 of their size."""
    return torch.equal(a, b) if exact else bool(((a - b).abs() <= 1e-12 * b.abs().max()).all())


@pytest.mark.parametrize("key", ["N128-rl4", "N96-c2c"])
def test_the_call_leaves_the_loop_alone(key, monkeypatch):
    """SH_step; step; sh_gradient; SH_step against the same sequence on a twin that makes no gradient call: step outputs bit for bit, the
    actions and get_state() bit for bit on the separable route (see _same_actions for the other).  Then sh_image .. sh_gradient ..
    sh_update(None): the image bit for bit, the update as _same_actions holds k_sh_estimate."""
    torch = _torch()
    env, _, _ = _make(key, monkeypatch)
    twin, _, _ = _make(key, monkeypatch)
    exact = key == "N128-rl4"
    B, ns = env.num_envs, env.sh.n_sub
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((B, 2 * ns))).cuda()
    grad = env.sh_gradient(g_slopes=g, actuators=torch.full((B, A), 1e-8, dtype=torch.float64, device="cuda:0"))
    assert float(grad.abs().max()) > 0
    a1, b1 = env.SH_step()[0], twin.SH_step()[0]
    assert _same_actions(torch, a1, b1, exact)
    so, st = env.step(b1.to(torch.float32)), twin.step(b1.to(torch.float32))
    env.sh_gradient(g_slopes=g)
    assert all(torch.equal(p, q) for p, q in zip(_flat(torch, so), _flat(torch, st))) and len(_flat(torch, so)) > 3
    assert _same_actions(torch, env.SH_step()[0], twin.SH_step()[0], exact)
    if exact:
        assert all(torch.equal(p, q) for p, q in zip(_flat(torch, env.get_state()), _flat(torch, twin.get_state())))
    assert torch.equal(env.sh_image(), twin.sh_image())
    env.sh_gradient(g_slopes=g, g_image=torch.ones((B, env.num_pupil_pixels ** 2), dtype=torch.float64, device="cuda:0"))
    assert _same_actions(torch, env.sh_update(None), twin.sh_update(None), False)
    env.close()
    twin.close()


@pytest.mark.parametrize("key", ["N128-rl4", "N96-c2c"])
def test_actuators_argument(key, monkeypatch):
    """``actuators=X`` equals the call on a twin whose sensor mirror stands at X (set through its checkpoint), and moves no mirror."""
    torch = _torch()
    env, _, act = _make(key, monkeypatch)
    twin, _, _ = _make(key, monkeypatch)
    twin.SH_step()
    x = twin.SH_step()[0].clone()      # where the twin's sensor mirror stands now
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((env.num_envs, 2 * env.sh.n_sub))).cuda()
    got = env.sh_gradient(g_slopes=g, actuators=x, with_values=True)
    want = twin.sh_gradient(g_slopes=g, with_values=True)
    assert all(torch.equal(p, q) for p, q in zip(got, want)) and not torch.equal(x, act)
    assert torch.equal(env.sh_gradient(g_slopes=g), env.sh_gradient(g_slopes=g, actuators=act)) and not torch.equal(got[0], env.sh_gradient(g_slopes=g))
    fresh = _make(key, monkeypatch)[0]
    assert _same_actions(torch, env.SH_step()[0], fresh.SH_step()[0], key == "N128-rl4")   # the integrator went on from `act`
    for e in (env, twin, fresh):
        e.close()


@pytest.mark.parametrize("key", ["N128-rl4", "N96-c2c", "N128-z2z"])
def test_masks_and_grouping_change_no_bit(key, monkeypatch):
    """Envs [0, 20) and [20, 33) on two handles reproduce the 33-env result bit for bit; masked-out rows read zero, the others keep their bits."""
    torch = _torch()
    B = MATRIX[key][1]
    r = np.random.default_rng(9)
    gi_all, gs_all = r.standard_normal((B, MATRIX[key][0] ** 2)), None

    def run(n, offset, mask=None):
        nonlocal gs_all
        env, _, _ = _make(key, monkeypatch, n=n, offset=offset)
        if gs_all is None:
            gs_all = r.standard_normal((B, 2 * env.sh.n_sub))
        res = env.sh_gradient(g_image=torch.from_numpy(gi_all[offset:offset + n]).cuda(), g_slopes=torch.from_numpy(gs_all[offset:offset + n]).cuda(),
                              mask=mask, with_values=True)
        torch.cuda.synchronize()
        env.close()
        return res

    whole = run(B, 0)
    assert float(whole[0].abs().max()) > 0
    halves = [run(20, 0), run(B - 20, 20)]
    for k in range(3):
        assert torch.equal(torch.cat([halves[0][k], halves[1][k]]), whole[k])
    sel = r.random(B) < 0.5
    sel[[0, B - 1]] = True, False
    masked = run(B, 0, mask=sel)
    keep = torch.from_numpy(sel).cuda()
    for k in range(3):
        assert torch.equal(masked[k][keep], whole[k][keep]) and bool((masked[k][~keep] == 0).all())


@pytest.mark.parametrize("key", ["N128-rl4", "N96-c2c"])
def test_side_stream(key, monkeypatch, cycles_per_ms):  # noqa: F811
    """The call on a caller's side stream behind a delayed producer equals the default-stream call bit for bit (stream_harness).  The first
    call makes the work buffers with blocking copies, like an upload; the calls after it are held to the harness's self-check."""
    B = MATRIX[key][1]

    def script(env, run):
        r = np.random.default_rng(4)
        ns = env.sh.n_sub
        g = run.input(np.ones((B, 2 * ns)))
        run.call("first call (allocates)", lambda: env.sh_gradient(g_slopes=g), blocking="upload")
        g, a = run.input(r.standard_normal((B, 2 * ns))), run.input(1e-8 * r.standard_normal((B, A)))
        run.call("sh_gradient", lambda: env.sh_gradient(g_slopes=g, actuators=a, with_values=True))
        a = run.input(1e-8 * r.standard_normal((B, A)))
        run.call("sh_clean", lambda: env.sh_clean(actuators=a))

    _both(cycles_per_ms, lambda: _make(key, monkeypatch)[0], script)


def test_autograd_sh_slopes_and_descent(monkeypatch):
    """torch.autograd.grad of 1/2 |s(a) - s_target|^2 through autograd.sh_slopes equals sh_gradient with the residual as cotangent; on the
    complex128 handle at N = 96, ten normalised gradient steps from a = 0 towards the slopes of a known command lower the loss every time."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, autograd

    N, B = 96, 3
    env = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, screens=smooth_screens(B, N, 5, amp=1e-5), sh_fft_precision="double", seed=3, **KW)
    env.reset()
    target_cmd = torch.from_numpy(2e-8 * np.random.default_rng(8).standard_normal((B, A))).cuda()
    with torch.no_grad():
        s_target = autograd.sh_slopes(env, target_cmd).clone()
    a = torch.zeros((B, A), dtype=torch.float64, device="cuda:0", requires_grad=True)
    s = autograd.sh_slopes(env, a)
    loss = 0.5 * ((s - s_target) ** 2).sum()
    (g,) = torch.autograd.grad(loss, a)
    assert torch.equal(g, env.sh_gradient(g_slopes=(s.detach() - s_target), actuators=a.detach()))
    img = autograd.sh_image(env, a)
    (g2,) = torch.autograd.grad(img.sum(), a)
    assert torch.equal(g2, env.sh_gradient(g_image=torch.ones_like(img), actuators=a.detach()))
    # ten gradient steps of length 1 / ||J||_2^2 (J by central differences of the clean slopes at a = 0: the loss is a quadratic to first
    # order, which such a step can only lower)
    eye = 1e-10 * torch.eye(A, dtype=torch.float64, device="cuda:0")
    zero = torch.zeros((B, A), dtype=torch.float64, device="cuda:0")
    J = torch.stack([(env.sh_clean(actuators=zero + eye[k])[1] - env.sh_clean(actuators=zero - eye[k])[1]) / 2e-10 for k in range(A)], dim=2)
    eta = 1.0 / torch.linalg.matrix_norm(J, ord=2) ** 2
    x, losses = zero.clone(), []
    for _ in range(11):
        r0 = env.sh_clean(actuators=x)[1] - s_target
        losses.append(float(0.5 * (r0 ** 2).sum()))
        x = x - eta[:, None] * env.sh_gradient(g_slopes=r0, actuators=x)
    print("gradient descent losses:", ["%.3e" % v for v in losses])
    assert losses[0] > 0 and all(b < a_ for a_, b in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0]
    out = autograd.sh_slopes(env, torch.zeros((B, A), dtype=torch.float64, device="cuda:0", requires_grad=True)).sum()
    env.reset()
    with pytest.raises(RuntimeError, match="stepped, reset or restored"):
        out.backward()
    env.close()


def test_refusals(monkeypatch):
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, _lib

    monkeypatch.delenv("AOG_SH_THREE_PASS", raising=False)
    n, N = 5, 96
    kw = dict(num_pupil_pixels=N, screens=smooth_screens(n, N, 2), **KW)
    p = lambda t: C.c_void_p(t.data_ptr())
    grad = torch.zeros((n, A), dtype=torch.float64, device="cuda:0")
    cot = torch.ones(n * N * N, dtype=torch.float64, device="cuda:0")
    # no SH_operation: the wrapper says so, and the library refuses before anything is allocated
    plain = BatchedAOEnv(n, "cuda:0", **{**kw, "SH_operation": False})
    base = plain.device_bytes()
    with pytest.raises(ValueError, match="Shack-Hartmann sensor"):
        plain.sh_gradient(g_slopes=cot[:n])
    assert plain.lib.aog_sh_gradient(plain._handle, None, p(cot), None, None, p(grad), None, None, None) == -3
    assert b"not uploaded" in plain.lib.aog_last_error() and plain.device_bytes() == base
    plain.close()
    env = BatchedAOEnv(n, "cuda:0", **kw)
    env.reset()
    ns = env.sh.n_sub
    acts = torch.from_numpy(1e-8 * np.random.RandomState(6).randn(2, n, A).astype(np.float32)).cuda()
    env.step(acts[0], next_actions=acts[1])   # (a pipelined pair first: what the step path allocates on first use is there)
    env.step(acts[1], next_actions=None)
    env._upload_gradient()                    # (the output gradient's tables, which the wrapper uploads before it calls: not this call's buffers)
    before = env.device_bytes()
    with pytest.raises(ValueError, match="at least one of g_image and g_slopes"):
        env.sh_gradient()
    assert env.lib.aog_sh_gradient(env._handle, None, None, None, None, p(grad), None, None, None) == -1 and b"cotangent" in env.lib.aog_last_error()
    assert env.lib.aog_sh_gradient(env._handle, None, p(cot), None, None, None, None, None, None) == -1
    with pytest.raises(ValueError, match="g_slopes must have shape"):
        env.sh_gradient(g_slopes=torch.zeros((n, 2 * ns + 1)))
    with pytest.raises(ValueError, match="g_image must have shape"):
        env.sh_gradient(g_image=torch.zeros((n, N * N - 1)))
    with pytest.raises(ValueError, match="actuators must have shape"):
        env.sh_clean(actuators=torch.zeros((n, A + 1)))
    g = torch.ones((n, 2 * ns), dtype=torch.float64, device="cuda:0")
    env.step(acts[0], next_actions=acts[1])   # a pending action: the mirror already belongs to the next step
    with pytest.raises(_lib.AogError, match="libaogym error -3"):
        env.sh_gradient(g_slopes=g)
    env.step(acts[1], next_actions=None)
    assert env.device_bytes() == before       # nothing was allocated by the refused calls
    assert float(env.sh_gradient(g_slopes=g).abs().max()) > 0 and env.device_bytes() > before
    env.close()
    # between two steps of a lookahead episode
    dyn = BatchedAOEnv(n, "cuda:0", atm_type="dynamic", atm_vel=20.0, num_pupil_pixels=N, **KW)
    assert dyn.lookahead(True)
    dyn.reset()
    dyn.step(torch.zeros((n, A), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(_lib.AogError, match="libaogym error -3"):
        dyn.sh_gradient(g_slopes=torch.ones((n, 2 * dyn.sh.n_sub), dtype=torch.float64, device="cuda:0"))
    assert b"aog_set_lookahead" in dyn.lib.aog_last_error()
    dyn.close()
