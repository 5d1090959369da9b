"""Tomography on the device: aog_wavefront_project against the host restatement (tests/tomography_reference.py), a poke that pins the
units, aog_tomo_update against its bit-exact replay, the least-squares ceiling and the closed loop on stand-alone pieces (static fronts,
aog_install_layer_sum_conjugate, AltitudeMirror), and ``TomographicController`` through ``LayeredAOEnv`` and ``rollout``.

Shapes: N = 32 under a meta-pupil of 44, A = 6 Zernike modes (the first is piston), one 3 x 3 mirror at 1e4 m, B in {5, 33} (33 crosses
an env tile of 32); n_ap = 812 = 25 pixel tiles and a ragged 26th.  K = 130 shapes are 5 blocks of 32 rows: two row groups of 3 blocks,
the last one ragged."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import conjugate_reference as cref
import tomography_reference as ref
import wavefront_reference as wr
from test_gpu_conjugate import MIRRORS, _install, _mirror
from test_gpu_disturbance import _static_env
from test_gpu_layered import _kw, _layers, _step_tensors
from test_gpu_parity import _torch

pytestmark = pytest.mark.gpu

N, NL, A = 32, 44, 6
# fast handles, as a fraction of max_k |out[b]|: the bound tests/test_gpu_wavefront_truth.py holds coef to — the same chain of arithmetic
PARITY = 1e-5
LOOKS = [(2.25, -1.5), (-3.5, 0.75)]     # (sx, sy) of layer and mirror at 1e4 m on the two guide fronts: fractional, inside the margin of 6
BATCHES = [5, 33]


def _np(t):
    return t.cpu().numpy()


def _front(B, precision, screens=None, act=None):
    torch = _torch()
    env = _static_env(B, N=N, precision=precision)
    if screens is not None:
        env.set_screens(screens)
    if act is not None:
        env.set_actuators(torch.from_numpy(act).cuda())
    return env


def _layer(B, screens):
    from adaptive_optics_gym_amd import BatchedAOEnv, OpticalParams

    params = dataclasses.replace(OpticalParams(num_pupil_pixels=N), num_pupil_pixels=NL, telescope_diameter=0.5 * NL / N)
    layer = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30.0, atm_fried=0.15, seed=3, params=params, **_kw(N=NL, T=0))
    layer.set_screens(screens)
    return layer


def _look(B, look):
    """[2, B, 2]: layer and mirror at one altitude read at one shift, the same for every env."""
    return np.tile(np.asarray(look, dtype=np.float64)[None, None, :], (2, B, 1))


def _host_w(env):
    return wr.path_error(_np(env.get_screens()), _np(env.get_actuators()), env.tables)


# ---- 1. the projection -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fp64"])
@pytest.mark.parametrize("B", BATCHES)
def test_project_matches_the_restatement(B, precision):
    """Float64 handles: within 8 n_ap 2^-53 sum_p |S| |w| (the header's bound on one order of the sum, and as much again for w itself).
    Fast handles: PARITY x max_k |out[b]|."""
    torch = _torch()
    from adaptive_optics_gym_amd import tomography as tm

    rng = np.random.RandomState(B)
    env = _front(B, precision, screens=rng.randn(B, N, N) * 2 * np.pi * 1e-7, act=rng.randn(B, A) * 5e-8)
    n_ap = int(env.tables.n_ap)
    w = _host_w(env)
    worst = 0.0
    for K, size in ((3, 1.0), (15, 3.7e-3), (130, 250.0)):      # (sizes far from one: the operand scale is the upload's)
        S = rng.randn(K, n_ap) * size
        S[0] += 0.5 * size                                       # a shape with a mean: the centring is the row sum's work
        tm.upload_wavefront_shapes(env, S)
        mean = torch.empty((B,), dtype=torch.float64, device="cuda")
        got = _np(tm.wavefront_project(env, mean=mean))
        want, want_mean, scale64 = ref.project(S, w)
        assert got.shape == (B, K)
        err = np.abs(got - want)
        if precision == "fp64":
            print(f"B={B} K={K} fp64: worst |error| / (n_ap eps sum|S||w|) = {np.max(err / scale64):.3g}")
            assert np.all(err <= 8 * scale64)
            np.testing.assert_allclose(_np(mean), want_mean, rtol=0, atol=1e-12 * np.abs(w).max())
        else:
            rel = float(np.max(err.max(axis=1) / np.abs(want).max(axis=1)))
            worst = max(worst, rel)
            print(f"B={B} K={K} fast: worst |error| / max_k |out| = {rel:.3g}")
            assert rel <= PARITY
            np.testing.assert_allclose(_np(mean), want_mean, rtol=0, atol=PARITY * np.abs(w).max())
    # the modes as shapes: out is the Mc' w that wavefront_truth's coef = fit (Mc' w) is built from
    modes = np.asarray(env.tables.modes, dtype=np.float64)
    tm.upload_wavefront_shapes(env, modes.T)
    out = _np(tm.wavefront_project(env))
    Mc = modes - modes.mean(axis=0)
    back = _np(env.wavefront_truth()["coef"]) @ (Mc.T @ Mc)       # (fit = pinv(Mc' Mc): its inverse on everything but the piston mode)
    rel = float(np.max(np.abs(out - back).max(axis=1) / np.abs(out).max(axis=1)))
    print(f"B={B} {precision}: modes as shapes against fit^-1 coef: {rel:.3g}")
    assert rel <= (PARITY if precision == "fast" else 1e-10)
    env.close()


def test_a_split_batch_projects_to_the_same_bits():
    from adaptive_optics_gym_amd import tomography as tm

    rng = np.random.RandomState(2)
    B = 66
    screens, act = rng.randn(B, N, N) * 2 * np.pi * 1e-7, rng.randn(B, A) * 5e-8
    whole = _front(B, "fast", screens, act)
    S = rng.randn(130, int(whole.tables.n_ap))
    tm.upload_wavefront_shapes(whole, S)
    want = tm.wavefront_project(whole)
    for lo, hi in ((0, 33), (33, 66)):
        part = _front(hi - lo, "fast", screens[lo:hi], act[lo:hi])
        tm.upload_wavefront_shapes(part, S)
        assert _torch().equal(tm.wavefront_project(part), want[lo:hi])
        part.close()
    whole.close()


# ---- 2. a poke pins the units ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fp64"])
@pytest.mark.parametrize("B", BATCHES)
def test_a_poke_answers_with_a_column_of_the_normal_matrix(B, precision):
    from adaptive_optics_gym_amd import tomography as tm
    from adaptive_optics_gym_amd.conjugate import influence_basis

    basis = influence_basis(NL, 3)
    layer, m, front = _layer(B, np.zeros((B, NL, NL))), _mirror(B, NL, basis), _front(B, precision)
    T = tm.sightline_shapes(front, [m], [LOOKS[0]])
    Tc = tm.centred(T)
    tm.upload_wavefront_shapes(front, Tc)
    assert _install(front, [layer], [m], _look(B, LOOKS[0]))[0] == 0
    rest = _np(tm.wavefront_project(front))
    e, k, c = B - 2, 4, 1e-7
    cmd = np.zeros((B, 9))
    cmd[e, k] = c
    m.set_command(cmd)
    assert _install(front, [layer], [m], _look(B, LOOKS[0]))[0] == 0
    diff = _np(tm.wavefront_project(front)) - rest
    want = c * (Tc @ Tc.T)[:, A + k]
    bound = (PARITY if precision == "fast" else 1e-10) * np.abs(want).max()
    print(f"B={B} {precision}: poke response deviates {np.abs(diff[e] - want).max() / np.abs(want).max():.3g} of its largest entry")
    assert np.all(np.abs(diff[e] - want) <= bound)
    others = np.delete(diff, e, axis=0)
    assert not others.any()      # (an env's sums depend on its own column alone)
    for x in (layer, m, front):
        x.close()


# ---- 3. the integrator -------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(_np(x) if hasattr(x, "cpu") else x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("B,K,widths", [(5, 15, (15, 6)), (33, 15, (15, 6)), (33, 70, (130, 6))], ids=["B5", "B33", "B33-K70-J130"])
def test_update_equals_the_replay_bit_for_bit(B, K, widths):
    """K = 15 and widths 15 and 6: one output tile and one column chunk.  K = 70 with 130 columns: a second output tile (ragged, 6 of 64) and
    three column chunks of the staging loop, the last one ragged (2 of 64)."""
    torch = _torch()
    from adaptive_optics_gym_amd.tomography import DeviceTomograph

    rng = np.random.RandomState(40 + B + K)
    gain, leak, stroke = 0.5, 0.99, 6e-8 * np.sqrt(sum(widths) / 21.0)
    R = [rng.randn(K, J) for J in widths]
    parts = [(0, B)] + ([(0, 20), (20, 33)] if B == 33 else [])
    handles = [DeviceTomograph(hi - lo, K, widths, env_id_base=lo) for lo, hi in parts]
    for h in handles:
        for g, r in enumerate(R):
            h.upload(g, r)
    u = np.zeros((B, K))
    clipped = 0
    for step in range(3):
        s = [rng.randn(B, J) * 1e-7 for J in widths]
        s[0][::3, 1] = 0.0
        mask = None if step == 0 else (np.arange(B) + step) % 3 != 0
        u = ref.update(u, R, s, gain, leak, stroke, mask)
        clipped += int(np.count_nonzero(np.abs(u) == stroke))
        for h, (lo, hi) in zip(handles, parts):
            out = h.update([torch.from_numpy(x[lo:hi].copy()).cuda() for x in s], gain, leak, stroke, None if mask is None else torch.from_numpy(mask[lo:hi]).cuda())
            np.testing.assert_array_equal(_bits(out), _bits(u[lo:hi]), err_msg=f"step {step}, envs {lo}:{hi}")
            np.testing.assert_array_equal(_bits(h.command), _bits(u[lo:hi]))
    assert 0 < clipped < u.size * 3
    # the state is u; reset(mask) zeroes the masked envs alone
    h = handles[0]
    other = DeviceTomograph(B, K, widths)
    other.set_state(h.get_state())
    np.testing.assert_array_equal(_bits(other.command), _bits(u))
    mask = np.arange(B) % 2 == 0
    h.reset(torch.from_numpy(mask).cuda())
    got = _np(h.command)
    assert not got[mask].any()
    np.testing.assert_array_equal(_bits(got[~mask]), _bits(u[~mask]))
    for x in handles + [other]:
        x.close()


# ---- 4. and 5. the ceiling and the loop, on stand-alone pieces ---------------------------------------------------------------------------------
class _Rig:
    """One layer at 1e4 m whose screens are sum_k c_k basis_k, a flat mirror at the same altitude and two float64 guide fronts at LOOKS."""

    def __init__(self, B, measurement="truth", pupil_mirror=False, looks=LOOKS, **kw):
        from adaptive_optics_gym_amd import tomography as tm
        from adaptive_optics_gym_amd.conjugate import influence_basis

        self.B, self.looks = B, list(looks)
        self.basis = influence_basis(NL, 3)
        self.c = np.random.RandomState(8).randn(B, 9) * 1e-7
        self.layer = _layer(B, cref.surface(self.c, self.basis).reshape(B, NL, NL))
        self.mirror = _mirror(B, NL, self.basis)
        self.fronts = [_front(B, "fp64") for _ in self.looks]
        self.ctrl = tm.TomographicController.from_parts(self.fronts, [self.mirror], [[look] for look in self.looks], measurement=measurement,
                                                        pupil_mirror=pupil_mirror, **kw)
        self.install()

    def install(self):
        for front, look in zip(self.fronts, self.looks):
            rc, msg = _install(front, [self.layer], [self.mirror], _look(self.B, look))
            assert rc == 0, msg

    def rms(self):
        return np.stack([_np(f.wavefront_truth()["rms"]) for f in self.fronts])

    def close(self):
        self.ctrl.close()
        for x in self.fronts + [self.layer, self.mirror]:
            x.close()


@pytest.mark.parametrize("B", BATCHES)
def test_the_ceiling_is_the_least_squares(B):
    """``fit()`` through the normal equations, restated in numpy (``tomography_reference.fit``) on the same inputs, leaves a relative error
    of 3.5e-12 of max |c| at B = 5 and 3.4e-12 at B = 33 (computed on the host; cond(H) = 3.4e4 for this geometry, and the SVD route
    ``tomography_reference.least_squares`` leaves 3.6e-15): the device is held to ten times the figure the restatement leaves here."""
    rig = _Rig(B, alpha=0.0)
    ctrl, c = rig.ctrl, rig.c
    T = ctrl.T
    assert np.linalg.cond(ref.normal_matrix(T, [1.0, 1.0])) < 1e8
    w = [_host_w(f) for f in rig.fronts]
    host = ref.fit(np.zeros((B, 9)), T, [1.0, 1.0], 0.0, w)
    figure = np.abs(host + c).max() / np.abs(c).max()
    flat = rig.rms()
    u = ctrl.fit()
    got = np.abs(_np(u) + c).max() / np.abs(c).max()
    print(f"B={B}: fit() leaves {got:.3g} of max |c|, the numpy restatement {figure:.3g}")
    assert figure < 1e-10 and got <= 10 * figure
    assert not _np(rig.mirror.command).any() and not _np(ctrl.command).any()      # fit() wrote no state
    rig.mirror.set_command(u)
    rig.install()
    left = rig.rms()
    print(f"B={B}: residual rms / flat rms up to {np.max(left / flat):.3g} on the two fronts")
    assert np.all(flat > 1e-9) and np.all(left < 1e-6 * flat)
    rig.close()
    # with the pupil mirror among the unknowns: the normal equations are solved
    torch = _torch()
    rig = _Rig(B, alpha=0.0, pupil_mirror=True)
    act = np.random.RandomState(9).randn(B, A) * 3e-8
    for f in rig.fronts:
        f.set_actuators(torch.from_numpy(act).cuda())
    before = _np(rig.ctrl.normal_residual())
    u = rig.ctrl.fit()
    for f in rig.fronts:
        f.set_actuators(u[:, :A].contiguous())
    rig.mirror.set_command(u[:, A:].contiguous())
    rig.install()
    after = _np(rig.ctrl.normal_residual())
    ratio = np.linalg.norm(after, axis=1) / np.linalg.norm(before, axis=1)
    print(f"B={B}: |sum_g w_g b_g| after / before up to {ratio.max():.3g}")
    assert np.all(ratio < 1e-8)
    rig.close()


def _residual(rig):
    """The guide-direction residual: the rms over the guide fronts' apertures."""
    return np.sqrt((rig.rms() ** 2).mean(axis=0))


def _run(rig, n):
    """[n + 1, B]: the residual before and after each of n iterations of install, action(), install again (a frozen state)."""
    r = [_residual(rig)]
    for _ in range(n):
        rig.ctrl.action()
        rig.install()
        r.append(_residual(rig))
    return np.array(r)


def _modal_loop_on_the_host(rig, n, gain=0.5, alpha=1e-6):
    """The same residuals from the definitions alone, in numpy: s_g = D_g (c + u), u <- u - gain sum_g R_g s_g, residual^2 = the mean over
    the fronts and the aperture of ((c + u) Tc_g)^2."""
    from adaptive_optics_gym_amd import tomography as tm
    from adaptive_optics_gym_amd.optics_host import wavefront_fit

    tables = rig.fronts[0].tables
    modes = np.asarray(tables.modes, dtype=np.float64)
    T = [ref.shapes(modes, np.asarray(tables.ap_index), N, [rig.basis], [look], pupil_mirror=False) for look in rig.looks]
    Tc = [ref.centred(x) for x in T]
    D = [tm.modal_interaction(x, modes, wavefront_fit(modes)) for x in T]
    R = tm.modal_reconstructors(D, [1.0] * len(T), alpha)
    u = np.zeros_like(rig.c)
    r = []
    for _ in range(n + 1):
        r.append(np.sqrt(np.mean([(((rig.c + u) @ x) ** 2).mean(axis=1) for x in Tc], axis=0)))
        u = u - gain * sum(((rig.c + u) @ d.T) @ m.T for d, m in zip(D, R))
    return np.array(r)


@pytest.mark.parametrize("B", BATCHES)
def test_the_loop_closes(B):
    """The truth loop at gain 0.5 halves the guide-direction residual per iteration, and the modal loop follows its host restatement.

    "No smaller than truth's" is asserted where it is a statement that can fail.  On two guide fronts the mode-limited sensor returns
    2 x 5 numbers for the 9 unknowns and is full rank: both loops go to zero, and after equal iterations neither leads per env (after 8 the
    modal loop stands at 3.868e-3 .. 3.984e-3 of the start on the host against the truth loop's 2^-8 = 3.906e-3 — (1 - gain m)^n with
    m < 1 is slower in the sensor's eigenbasis, which is not the residual norm's), so there the modal loop is held to the host
    restatement instead.  On ONE guide front the sensor returns 5 numbers for 9 unknowns: the truth loop still goes to zero (2^-12 after
    12 iterations) and the modal loop stalls at 1.3 % .. 29 % of the start (host), which is the comparison asserted."""
    rig = _Rig(B, gain=0.5, alpha=0.0)
    r = _run(rig, 8)
    ratio = r[:-1] / r[1:]
    print(f"B={B} truth: residual falls by {ratio.min():.4f} .. {ratio.max():.4f} per iteration")
    assert np.all(np.abs(ratio - 2.0) <= 0.02)
    truth8 = r[-1] / r[0]
    rig.close()
    modal = _Rig(B, measurement="modal", gain=0.5)
    got, want = _run(modal, 8), _modal_loop_on_the_host(modal, 8)
    print(f"B={B}, two guide fronts, residual / start after 8 iterations: truth {truth8.min():.6g} .. {truth8.max():.6g}, "
          f"modal {np.min(got[-1] / got[0]):.6g} .. {np.max(got[-1] / got[0]):.6g} (host {np.min(want[-1] / want[0]):.6g} .. {np.max(want[-1] / want[0]):.6g})")
    # (float64 throughout; the device forms coef through the normal equations of the fit, the host through the same matrices)
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert np.all(got[-1] < 0.01 * got[0])
    modal.close()
    # one guide front: a rank-limited sensor stalls above the loop that sees the whole residual
    one = LOOKS[:1]
    rig = _Rig(B, gain=0.5, alpha=0.0, looks=one)
    truth = _run(rig, 12)
    rig.close()
    modal = _Rig(B, measurement="modal", gain=0.5, looks=one)
    got, want = _run(modal, 13), _modal_loop_on_the_host(modal, 13)
    print(f"B={B}, one guide front, residual / start after 12 iterations: truth {np.max(truth[-1] / truth[0]):.3g}, "
          f"modal {np.min(got[12] / got[0]):.3g} .. {np.max(got[12] / got[0]):.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert np.all(np.abs(truth[-1] / truth[0] - 2.0 ** -12) <= 0.02 * 2.0 ** -12)
    assert np.all(got[12] < got[0]) and np.all(np.abs(got[13] - got[12]) <= 1e-3 * got[12])      # it has converged ...
    assert np.all(got[12] >= truth[12])                                                            # ... to no less than the truth loop's
    modal.close()


# ---- 6. through the env ------------------------------------------------------------------------------------------------------------------------
UPLINK = (-4e-6, 1e-6)


def _layered(B, **kw):
    from adaptive_optics_gym_amd import LayeredAOEnv

    more = dict(A=A, T=4, SH_operation=True)
    more.update(kw)
    return LayeredAOEnv(B, "cuda:0", atm_layers=_layers(2), atm_fried=0.15, seed=11, layer_altitudes=[0.0, 1e4], altitude_mirrors=MIRRORS,
                        sightlines={"uplink": UPLINK}, **_kw(**more))


def _controller(env, **kw):
    from adaptive_optics_gym_amd.tomography import TomographicController

    return TomographicController(env, guide_stars=("self", "uplink"), **kw)


def _by_hand(env, ctrl, T):
    torch = _torch()
    rows = []
    obs = env.reset()[0]
    ctrl.reset()
    for t in range(T):
        a = ctrl.action().to(torch.float32)
        ret = env.step(a)
        rows.append([a.clone()] + [x.clone() for x in _step_tensors(ret)] + [env.altitude_mirrors[0].command.clone(), ret[4]["sightlines"]["uplink"]["power"].clone()])
    return obs.clone(), rows


@pytest.mark.parametrize("B", BATCHES)
def test_rollout_reproduces_the_loop_by_hand(B):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import rollout

    T = 4
    env, twin = _layered(B, T=T), _layered(B, T=T)
    ctrl, ctrl2 = _controller(env), _controller(twin)
    out = rollout(env, None, policy="tomographic", controller=ctrl)
    obs0, rows = _by_hand(twin, ctrl2, T)
    assert torch.equal(out["obs"][0], obs0)
    for t, row in enumerate(rows):
        assert torch.equal(out["act"][t], row[0]), f"step {t}: action"
        assert torch.equal(out["next_obs"][t], row[1]) and torch.equal(out["rew"][t], row[2]), f"step {t}"
    assert torch.equal(env.altitude_mirrors[0].command, twin.altitude_mirrors[0].command) and bool(env.altitude_mirrors[0].command.ne(0).any())
    assert torch.equal(ctrl.command, ctrl2.command)
    assert bool((out["log_prob"] == 1).all())
    # an env without the controller steps to the bits it stepped to before the controller existed: the shapes uploaded to its fronts and the
    # projection change nothing a step reads
    plain, probed = _layered(B, T=T), _layered(B, T=T)
    idle = _controller(probed)
    acts = [torch.from_numpy(np.random.RandomState(t).randn(B, A).astype(np.float32) * 3e-8).cuda() for t in range(2)]
    assert torch.equal(plain.reset()[0], probed.reset()[0])
    for a in acts:
        idle.fit()
        for x, y in zip(_step_tensors(plain.step(a)), _step_tensors(probed.step(a))):
            assert torch.equal(x, y)
    for x in (ctrl, ctrl2, idle, env, twin, plain, probed):
        x.close()


def test_split_batch_reproduces_the_whole_batch():
    torch = _torch()
    B, T = 38, 3
    mk = lambda n, off: _layered(n, T=T, global_env_offset=off, total_envs=B)
    envs = [mk(B, 0), mk(33, 0), mk(5, 33)]
    ctrls = [_controller(e, stroke=2e-7) for e in envs]
    runs = [_by_hand(e, c, T) for e, c in zip(envs, ctrls)]
    cat = lambda xs: torch.cat(list(xs), dim=0)
    assert torch.equal(runs[0][0], cat([runs[1][0], runs[2][0]]))
    for t in range(T):
        for k, x in enumerate(runs[0][1][t]):
            assert torch.equal(x, cat([runs[1][1][t][k], runs[2][1][t][k]])), f"step {t}, output {k}"
    for x in ctrls + envs:
        x.close()


def test_state_dict_resumes_bit_identically():
    torch = _torch()
    T = 4
    env, twin = _layered(5, T=T), _layered(5, T=T)
    ctrl, ctrl2 = _controller(env, leak=0.99), _controller(twin, leak=0.99)

    def steps(e, c, n):
        out = []
        for _ in range(n):
            a = c.action().to(torch.float32)
            ret = e.step(a)
            out.append([a.clone()] + [x.clone() for x in _step_tensors(ret)] + [e.altitude_mirrors[0].command.clone()])
        return out

    env.reset(), ctrl.reset()
    steps(env, ctrl, 2)
    saved, state = env.get_state(), ctrl.state_dict()
    want = steps(env, ctrl, 2)
    twin.reset()
    steps(twin, ctrl2, 1)                      # (somewhere else before the restore)
    twin.set_state(saved), ctrl2.load_state_dict(state)
    got = steps(twin, ctrl2, 2)
    for t, (x, y) in enumerate(zip(want, got)):
        for k, (p, q) in enumerate(zip(x, y)):
            assert torch.equal(p, q), f"step {t} after the restore, output {k}"
    other = _controller(env, measurement="modal")
    with pytest.raises(ValueError, match="measurement"):
        other.load_state_dict(state)
    # the geometry is read at construction: once a guide direction moves, the controller refuses instead of steering with a stale H
    env.sightlines["uplink"].set_angle((3e-6, 2e-6))
    for call in (ctrl.action, ctrl.fit):
        with pytest.raises(ValueError, match="guide star 'uplink' looks along another angle"):
            call()
    env.sightlines["uplink"].set_angle(UPLINK)
    ctrl.action()
    for x in (ctrl, ctrl2, other, env, twin):
        x.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    torch = _torch()
    from adaptive_optics_gym_amd import _lib
    from adaptive_optics_gym_amd import tomography as tm
    from test_gpu_wavefront_truth import _env, actions_for

    B, A20 = 5, 20
    env = _env(B, act_dim=A20, timesteps_per_episode=3)
    env.reset()
    out = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    # before an upload
    assert env.lib.aog_wavefront_project(env._handle, C.c_void_p(out.data_ptr()), None, env._stream()) == -3      # AOG_ERR_STATE
    assert b"aog_upload_wavefront_shapes" in env.lib.aog_last_error()
    with pytest.raises(_lib.AogError, match="no shapes"):
        tm.wavefront_project(env)
    # K outside its range
    n_ap = int(env.tables.n_ap)
    for K in (0, 513):
        s = np.zeros((max(K, 1), n_ap))
        assert env.lib.aog_upload_wavefront_shapes(env._handle, s.ctypes.data_as(C.c_void_p), K) == -1
        assert b"n_shapes" in env.lib.aog_last_error()
    bad = np.zeros((2, n_ap))
    bad[1, 5] = np.nan
    with pytest.raises(_lib.AogError, match=r"shapes\[1\]\[5\]"):
        tm.upload_wavefront_shapes(env, bad)
    tm.upload_wavefront_shapes(env, np.random.RandomState(0).randn(3, n_ap))
    ok = tm.wavefront_project(env)
    # an output the library would write past: made for another K, of another type, or not a mean of B values
    for bad_out, bad_mean, word in ((torch.zeros((B, 2), dtype=torch.float64, device="cuda"), None, "out"),
                                    (torch.zeros((B, 3), dtype=torch.float32, device="cuda"), None, "out"),
                                    (None, torch.zeros((B - 1,), dtype=torch.float64, device="cuda"), "mean")):
        with pytest.raises(ValueError, match=f"wavefront_project: {word} must be"):
            tm.wavefront_project(env, out=bad_out, mean=bad_mean)
    assert torch.equal(tm.wavefront_project(env, out=torch.zeros((B, 3), dtype=torch.float64, device="cuda")), ok)
    # while an action is pending after a pipelined step, like wavefront_truth
    a = [torch.from_numpy(actions_for(B, A20, t)).cuda() for t in range(2)]
    env.step(a[0], next_actions=a[1])
    with pytest.raises(RuntimeError, match="aog_wavefront_project"):
        tm.wavefront_project(env)
    env.step(a[1], next_actions=None)
    tm.wavefront_project(env)
    # new tables forget the shapes
    env.reset()
    env._upload_tables()
    assert env.lib.aog_wavefront_project(env._handle, C.c_void_p(out.data_ptr()), None, env._stream()) == -3
    tm.upload_wavefront_shapes(env, np.random.RandomState(0).randn(3, n_ap))
    assert torch.equal(tm.wavefront_project(env), ok)
    env.close()
