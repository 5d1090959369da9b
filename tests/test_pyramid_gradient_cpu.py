"""The pyramid sensor's gradient without a GPU: the host restatement (pyramid_gradient_reference.py) against central finite differences of
pyramid_reference.Sensor's own frames and slopes, its reverse chain against its dense Jacobian, the new symbol through header, binding and
library, and the argument checks ``BatchedAOEnv.pyramid_gradient`` makes on the host."""
import os
import re

import numpy as np
import pytest

import pyramid_gradient_reference as gref
import pyramid_reference as ref
from adaptive_optics_gym_amd.optics_host import build_tables
from adaptive_optics_gym_amd.params import OpticalParams

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N, A, WQ, NS = 32, 6, 8, 8
MODULATIONS = [(1, 0.0), (3, 1.5)]
# finite-difference steps in waves of lambda_wfs at the mirror's surface: the truncation error of a central difference falls as h^2, its
# rounding error grows as 2^-53 / h, and float64 meets 1e-6 of the largest entry somewhere between 1e-4 and 1e-7 of a wave
STEPS_WAVES = (1e-4, 1e-5, 1e-6, 1e-7)


def _setup(n_mod, r_mod):
    params = OpticalParams(num_pupil_pixels=N)
    tb = build_tables(params, "zernike", A, 2)
    lam = params.wavelength_wfs
    sensor = ref.Sensor(N, tb.ap_index, WQ, 2, NS, n_mod, r_mod)
    rng = np.random.default_rng(5 + n_mod)
    yy, xx = np.mgrid[0:N, 0:N] / N
    # a smooth screen of a fraction of a wave (phase x lambda, the units of the env's screens) and non-zero actuators
    screen = 2 * np.pi * lam * (0.21 * np.sin(2 * np.pi * (1.3 * xx + 0.4 * yy)) + 0.13 * np.cos(2 * np.pi * (0.7 * yy - 0.9 * xx) + 0.5))
    scale = np.abs(tb.modes).max()
    act = rng.uniform(-1, 1, A) * 0.05 * lam / scale
    return sensor, tb, lam, screen, act


def _outputs(sensor, tb, lam, screen, act):
    f = sensor.frame(ref.phase_rev(screen, tb.modes, act, tb.ap_index, lam))
    return f, sensor.slopes_of(f)


@pytest.mark.parametrize("n_mod,r_mod", MODULATIONS)
def test_restatement_against_finite_differences(n_mod, r_mod):
    """The dense Jacobians of frames and slopes against central differences of Sensor.frame / Sensor.slopes_of, N = 32, A = 6, w_q = n_s = 8:
    within 1e-6 of each Jacobian's largest entry at the best of the steps tried."""
    sensor, tb, lam, screen, act = _setup(n_mod, r_mod)
    Jf, Js = gref.jacobians(sensor, tb.modes, lam, ref.phase_rev(screen, tb.modes, act, tb.ap_index, lam))
    assert Jf.shape == (4, NS, NS, A) and Js.shape == (2 * sensor.valid.size, A)
    mode_scale = np.abs(tb.modes).max()
    best_f = best_s = np.inf
    for waves in STEPS_WAVES:
        h = waves * lam / mode_scale
        Ff, Fs = np.empty_like(Jf), np.empty_like(Js)
        for k in range(A):
            d = np.zeros(A)
            d[k] = h
            fp, sp = _outputs(sensor, tb, lam, screen, act + d)
            fm, sm = _outputs(sensor, tb, lam, screen, act - d)
            Ff[..., k] = (fp - fm) / (2 * h)
            Fs[:, k] = (sp - sm) / (2 * h)
        ef = float(np.abs(Ff - Jf).max() / np.abs(Jf).max())
        es = float(np.abs(Fs - Js).max() / np.abs(Js).max())
        print(f"n_mod {n_mod}: step {waves:g} waves: frames {ef:.3e}, slopes {es:.3e} of the largest entry")
        best_f, best_s = min(best_f, ef), min(best_s, es)
    assert best_f <= 1e-6 and best_s <= 1e-6


@pytest.mark.parametrize("n_mod,r_mod", MODULATIONS)
def test_reverse_chain_is_the_jacobian_transposed(n_mod, r_mod):
    """grad() (W, V, H, q) against cotangent x dense Jacobian: two orders of the same float64 sums, so rounding alone — 4096 terms per
    entry, held at 1e-11 of the largest |gradient|."""
    sensor, tb, lam, screen, act = _setup(n_mod, r_mod)
    Jf, Js = gref.jacobians(sensor, tb.modes, lam, ref.phase_rev(screen, tb.modes, act, tb.ap_index, lam))
    rng = np.random.default_rng(3)
    gf, gs = rng.standard_normal((4, NS, NS)), rng.standard_normal(2 * sensor.valid.size)
    f0, s0 = _outputs(sensor, tb, lam, screen, act)
    for kw, want in ((dict(g_frames=gf), gf.ravel() @ Jf.reshape(-1, A)), (dict(g_slopes=gs), gs @ Js),
                     (dict(g_frames=gf, g_slopes=gs), gf.ravel() @ Jf.reshape(-1, A) + gs @ Js)):
        g, frame, slopes = gref.grad(sensor, screen, tb.modes, act, lam, **kw)
        assert np.abs(g - want).max() <= 1e-11 * np.abs(want).max()
        assert np.array_equal(frame, f0) and np.array_equal(slopes, s0)


def test_the_symbol_is_declared_bound_and_exported():
    """aog_pyramid_gradient in the header, in _lib.py's table and in the library, at ABI 22."""
    from adaptive_optics_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "aogym.h")).read()
    assert re.search(r"\bint\s+aog_pyramid_gradient\s*\(", header)
    assert re.search(r"#define\s+AOG_ABI_VERSION\s+22\b", header)
    assert "aog_pyramid_gradient" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["aog_pyramid_gradient"]
    assert len(argtypes) == 9
    lib = _lib.load()
    assert hasattr(lib, "aog_pyramid_gradient")
    assert lib.aog_abi_version() == 22


def _host_env():
    """A BatchedAOEnv shell with the host fields pyramid_gradient's checks read and no handle: a check that fails raises before the first
    library call; one that passes would reach ``self.lib`` and raise AttributeError."""
    from adaptive_optics_gym_amd.batched_env import BatchedAOEnv
    from adaptive_optics_gym_amd.pyramid_host import pyramid_tables

    params = OpticalParams(num_pupil_pixels=N)
    tb = build_tables(params, "zernike", A, 2)
    env = object.__new__(BatchedAOEnv)
    env.num_envs, env.num_modes, env.device = 3, A, "cpu"
    env._pyramid = pyramid_tables(N, tb.n_ap, WQ, 2, NS, 1, 0.0)
    env._pyramid_uploaded = True
    import torch

    env._torch = torch
    return env


def test_host_argument_checks():
    torch = pytest.importorskip("torch")
    env = _host_env()
    nv = env._pyramid.n_valid
    with pytest.raises(ValueError, match="at least one"):
        env.pyramid_gradient()
    with pytest.raises(ValueError, match="g_frames"):
        env.pyramid_gradient(g_frames=torch.zeros(3, 4, NS, NS + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="g_frames"):
        env.pyramid_gradient(g_frames=torch.zeros(2, 4, NS, NS, dtype=torch.float64))
    with pytest.raises(ValueError, match="g_slopes"):
        env.pyramid_gradient(g_slopes=torch.zeros(3, 2 * nv + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="actuators"):
        env.pyramid_gradient(g_slopes=torch.zeros(3, 2 * nv, dtype=torch.float64), actuators=torch.zeros(3, A + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="actuators"):
        env.pyramid_gradient(g_slopes=torch.zeros(3, 2 * nv, dtype=torch.float64), actuators=torch.zeros(A, dtype=torch.float64))
    no_sensor = _host_env()
    no_sensor._pyramid = None
    with pytest.raises(ValueError, match="without a pyramid sensor"):
        no_sensor.pyramid_gradient(g_slopes=torch.zeros(3, 2 * nv, dtype=torch.float64))
