"""Scintillation on the device (include/aogym_scintillation.h): aog_scint_filter, aog_scint_install and aog_scint_receive against the
float64 restatement (tests/scintillation_reference.py), and ``LayeredAOEnv(scintillation=...)`` on top of them.

Shapes: N = 32 (812 aperture pixels = 26 pixel tiles: the one pixel chunk holds fewer than four tiles per wave's last round, the last tile
is ragged) and N = 64, two layers at (0, 10 km), an off-axis sightline with a fractional-pixel shift, B = 3 and B = 33 (one env past a
32-env tile).  A guard of 4 pixels keeps the meta-pupils small: the edge error is the CPU test's subject, not this file's."""
import numpy as np
import pytest

import scintillation_reference as ref
import sightline_reference as sref
from test_gpu_layered import _actions, _kw, _layers
from test_gpu_parity import _torch

pytestmark = pytest.mark.gpu

ALTITUDES = (0.0, 1e4)
OWN, UP = (2e-6, -1e-6), (3.3e-6, 1.7e-6)
# profiles/scintillation.md: the worst |device - numpy| of a filtered surface over the surface's largest value on these shapes
RECORDED_FILTER_ERROR = 2.4e-14
FILTER_TOL = min(8 * RECORDED_FILTER_ERROR, 1e-10)


def _env(B, N=32, scint=True, altitudes=ALTITUDES, offset=0, total=None, T=8, sightline=True, **more):
    from adaptive_optics_gym_amd import LayeredAOEnv

    return LayeredAOEnv(B, "cuda:0", atm_layers=_layers(2), atm_fried=0.15, seed=11, layer_altitudes=list(altitudes), field_angle=OWN,
                        sightlines={"up": UP} if sightline else None, scintillation=dict(guard=4) if scint else None, global_env_offset=offset,
                        total_envs=total, **more, **_kw(N=N, A=6, T=T))


def _scint(info):
    return {k: v.clone() for k, v in info["scintillation"].items()}


def _same(a, b):
    return all(_torch().equal(a[k].view(_torch().int64), b[k].view(_torch().int64)) for k in a)


def _reference(env, front, shifts):
    """The receiver's float64 dict for ``front`` (the env or a sightline's front) from the layers' screens, the device's filtered surfaces
    (held to numpy's by test_filter_and_maps), the front's actuators and the host tables."""
    sc = env.scintillation
    ap, N, lam = np.asarray(env.tables.ap_index), env.num_pupil_pixels, env.params.wavelength_wfs
    corr, chi = (t.cpu().numpy() for t in sc.surfaces(0))
    screens = [env.layer_screens(l).cpu().numpy() for l in range(env.num_layers)]
    ext = np.concatenate([shifts, shifts[sc.layer_index]])
    psi = sref.install(screens + [corr], ext, ap, N, lam)["psi64"]
    u = psi / (2.0 * np.pi * lam) + 2.0 * front.get_actuators().cpu().numpy() @ np.asarray(env.tables.modes, dtype=np.float64).T / lam
    chi_ap = ref.chi_map([chi], shifts[sc.layer_index], ap, N, lam)
    from adaptive_optics_gym_amd.scintillation import receive_modes

    return ref.receive(u, chi_ap.astype(np.float64), receive_modes(env.tables)), chi_ap


@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("B", [3, 33])
def test_filter_and_maps(B, N):
    """aog_scint_filter's two surfaces against numpy on the same table (hipFFT is not numpy's transform: the measured worst relative error
    is in profiles/scintillation.md, asserted at 8x and never looser than 1e-10 of the surface's largest value); then the chi maps: bit for
    bit the restatement's bilinear read of the device's own surfaces, and the float32 rounding of the reference's values."""
    torch = _torch()
    env = _env(B, N)
    try:
        env.step(_actions(torch, 1, B, 6)[0])
        sc = env.scintillation
        corr, chi = (t.cpu().numpy() for t in sc.surfaces(0))
        screen = env.layer_screens(1).cpu().numpy()
        S_ref, chi_ref = ref.filter_layer(screen, sc.table[0])
        corr_ref = S_ref - screen
        errs = [np.abs(corr - corr_ref).max() / np.abs(corr_ref).max(), np.abs(chi - chi_ref).max() / np.abs(chi_ref).max()]
        print(f"B = {B}, N = {N}, M = {sc.n_pixels}: filter error over the largest value: S - phi {errs[0]:.3e}, chi {errs[1]:.3e}")
        assert max(errs) <= FILTER_TOL
        ap, lam = np.asarray(env.tables.ap_index), env.params.wavelength_wfs
        for front, shifts, got in ((env, env._shifts, env.log_amplitude()),
                                   (env.sightlines["up"].env, env.sightlines["up"]._shifts, sc.unpack_tile(env.sightlines["up"].env, env.sightlines["up"].env._chi_tile))):
            got = got.cpu().numpy().reshape(B, -1)
            assert (shifts[1] != np.floor(shifts[1])).all()
            own = ref.chi_map([chi], shifts[sc.layer_index], ap, N, lam)
            assert np.array_equal(got[:, ap].view(np.int32), own.view(np.int32))
            outside = np.setdiff1d(np.arange(N * N), ap)
            assert not got[:, outside].any()
            want = ref.chi_map([chi_ref], shifts[sc.layer_index], ap, N, lam).astype(np.float64)
            assert np.abs(got[:, ap] - want).max() <= 2.0 ** -23 * np.abs(want).max()
        tile = env._chi_tile.cpu().numpy()
        assert np.count_nonzero(tile) <= B * ap.size      # pad pixels and pad envs are zeros
    finally:
        env.close()


def test_opt_in_is_free():
    """Every layer at h = 0: nothing is filtered, the step is the step without the option bit for bit, and the receiver sees unit amplitude."""
    torch = _torch()
    B, T = 33, 3
    acts = _actions(torch, T, B, 6)
    runs = []
    for scint in (False, True):
        env = _env(B, 32, scint=scint, altitudes=(0.0, 0.0), sightline=False)
        try:
            env.reset()
            rows = []
            for t in range(T):
                obs, rew, _, _, info = env.step(acts[t])
                rows.append([obs.clone(), rew.clone(), info["power"].clone(), info["strehl"].clone()])
                if scint:
                    s = info["scintillation"]
                    assert torch.equal(s["irradiance"], torch.ones_like(s["irradiance"])) and not s["sigma_chi2"].any()
                    assert torch.allclose(s["power"], info["power"].double(), rtol=1e-5, atol=0)
                else:
                    assert "scintillation" not in info
            runs.append(rows)
        finally:
            env.close()
    for a, b in zip(*runs):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B, N", [(3, 32), (33, 32), (33, 64)])
def test_receiver_against_float64(B, N):
    """chi forced to zero: the step's own power (the project's parity tolerance, rtol 1e-5) for random actuators.  Zero actuators are not a
    state a step of this env can leave (it scales every action to the surface rms target, and a zero action divides by zero, with or
    without the option), so that case is the flat mirror a reset leaves, held to the float64 restatement's power instead.  The real chi:
    power, irradiance, strehl and sigma_chi2 against the float64 restatement at rtol 1e-5, on the env's front and on the sightline's."""
    torch = _torch()
    env = _env(B, N)
    try:
        env.reset()
        assert not env.get_actuators().any()
        flat = env.scintillation.receive(env, None)
        want, _ = _reference(env, env, env._shifts)
        from adaptive_optics_gym_amd.scintillation import receive_modes

        ap, lam = np.asarray(env.tables.ap_index), env.params.wavelength_wfs
        screens = [env.layer_screens(l).cpu().numpy() for l in range(2)] + [env.scintillation.surfaces(0)[0].cpu().numpy()]
        psi = sref.install(screens, np.concatenate([env._shifts, env._shifts[1:2]]), ap, N, lam)["psi64"]
        unit = ref.receive(psi / (2.0 * np.pi * lam), np.zeros_like(psi), receive_modes(env.tables))
        assert np.allclose(flat["power"].cpu().numpy(), unit["power"], rtol=1e-5, atol=0)
        acts = _actions(torch, 2, B, 6)
        for t, a in enumerate(acts):
            info = env.step(a)[4]
            flat = env.scintillation.receive(env, None)
            assert torch.allclose(flat["power"], info["power"].double(), rtol=1e-5, atol=0), t
            assert torch.equal(flat["irradiance"], torch.ones_like(flat["irradiance"])) and not flat["sigma_chi2"].any()
            up = env.sightlines["up"]
            for name, front, shifts, got in (("own", env, env._shifts, info["scintillation"]), ("up", up.env, up._shifts, info["sightlines"]["up"]["scintillation"])):
                want, chi_ap = _reference(env, front, shifts)
                for k in ("power", "irradiance", "strehl", "sigma_chi2"):
                    g = got[k].cpu().numpy()
                    print(f"step {t}, {name}, {k}: worst relative error {np.abs(g / want[k] - 1).max():.2e}")
                    assert np.allclose(g, want[k], rtol=1e-5, atol=0), (t, name, k)
                assert (want["sigma_chi2"] > 1e-3).all() and np.abs(want["irradiance"] - 1).max() > 1e-3     # (there is amplitude to see)
    finally:
        env.close()


def test_split_batch_is_bit_identical():
    torch = _torch()
    B, T = 33, 2
    acts = _actions(torch, T, B, 6)

    def run(n, off):
        env = _env(n, 32, offset=off, total=B)
        try:
            env.reset()
            out = []
            for t in range(T):
                info = env.step(acts[t, off:off + n])[4]
                out.append((_scint(info), {k: v.clone() for k, v in info["sightlines"]["up"]["scintillation"].items()}, env.log_amplitude().clone()))
            return out
        finally:
            env.close()

    whole, parts = run(B, 0), [run(16, 0), run(17, 16)]
    for t in range(T):
        for j in range(2):
            for k in whole[t][j]:
                joined = torch.cat([parts[0][t][j][k], parts[1][t][j][k]])
                assert torch.equal(whole[t][j][k].view(torch.int64), joined.view(torch.int64)), (t, j, k)
        assert torch.equal(whole[t][2], torch.cat([parts[0][t][2], parts[1][t][2]]))


def test_resume_and_side_stream_reproduce_the_run():
    """get_state / set_state carry nothing of the scintillation: a resume after 3 steps filters the restored screens again and gives the
    uninterrupted run's bits; so does the whole run on a caller's side stream."""
    torch = _torch()
    B, T = 3, 5
    acts = _actions(torch, T, B, 6)

    def steps(env, ts):
        out = []
        for t in ts:
            info = env.step(acts[t])[4]
            out.append((_scint(info), env.log_amplitude().clone()))
        return out

    base = _env(B, 32)
    try:
        base.reset()
        want = steps(base, range(T))
    finally:
        base.close()
    first = _env(B, 32)
    second = _env(B, 32)
    try:
        first.reset()
        steps(first, range(3))
        state = first.get_state()
        assert not any("scint" in str(k) or "chi" in str(k) for k in state)
        second.set_state(state)
        got = steps(second, range(3, T))
        for (a, amap), (b, bmap) in zip(want[3:], got):
            assert _same(a, b) and torch.equal(amap, bmap)
    finally:
        first.close()
        second.close()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _env(B, 32)
        try:
            env.reset()
            got = steps(env, range(T))
            side.synchronize()
        finally:
            env.close()
    for (a, amap), (b, bmap) in zip(want, got):
        assert _same(a, b) and torch.equal(amap, bmap)


def test_aperture_averaging():
    """Over 64 steps of the dynamic two-layer env the variance of the aperture's irradiance is below the point scintillation index, the
    mean over aperture pixels of the variance of exp(2 chi)."""
    torch = _torch()
    B, T = 3, 64
    env = _env(B, 32, T=T, sightline=False)
    try:
        env.reset()
        acts = _actions(torch, T, B, 6)
        ap = torch.from_numpy(np.asarray(env.tables.ap_index, dtype=np.int64)).cuda()
        irr, point = [], []
        for _ in range(T):
            info = env.step(acts[_])[4]
            irr.append(info["scintillation"]["irradiance"].clone())
            point.append(torch.exp(2.0 * env.log_amplitude().reshape(B, -1)[:, ap].double()))
        irr, point = torch.stack(irr), torch.stack(point)
        aperture, index = irr.var(dim=0), point.var(dim=0).mean(dim=1)
        print(f"irradiance variance {aperture.tolist()}, point scintillation index {index.tolist()}")
        assert (aperture < index).all() and (index > 0).all()
    finally:
        env.close()


def test_fused_and_pipelined_forms_are_refused():
    torch = _torch()
    env = _env(3, 32, sightline=False)
    try:
        env.reset()
        a = torch.zeros((3, 6), device="cuda")
        with pytest.raises(RuntimeError, match="scintillation"):
            env.step(a, next_actions=a)
        with pytest.raises(RuntimeError, match="scintillation"):
            env.step_with_policy(None)
        assert env.rytov_variance().shape == (3,) and (env.rytov_variance() > 0).all()
    finally:
        env.close()
