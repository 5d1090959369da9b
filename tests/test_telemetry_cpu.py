"""The modal telemetry without a device: the C-ABI surface, known answers of the numpy restatement (tests/telemetry_reference.py) and every
argument refusal, which comes before any handle exists."""
import math
import os
import re

import numpy as np
import pytest

import telemetry_reference as ref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd import telemetry as tel

TEL_SYMBOLS = ("aog_telemetry_create", "aog_telemetry_destroy", "aog_telemetry_reset", "aog_telemetry_push", "aog_telemetry_psd", "aog_telemetry_gains",
               "aog_telemetry_state_bytes", "aog_telemetry_get_state", "aog_telemetry_set_state")


def test_cabi_surface_lists_the_telemetry_entry_points(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    lib = _lib.load()
    for name in TEL_SYMBOLS:
        assert re.search(r"\b(int|void|int64_t)\s+%s\s*\(" % name, header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define AOG_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, header) and lib.aog_abi_version() == _lib.ABI_VERSION
    import ctypes as C

    assert C.sizeof(_lib.AogTelemetryConfig) == 16
    # argument checks that need no device
    for name, args in (("aog_telemetry_create", (None, 0, None)), ("aog_telemetry_reset", (None, None, None)), ("aog_telemetry_push", (None,) * 4),
                       ("aog_telemetry_psd", (None, 32, None, None, None, None)), ("aog_telemetry_gains", (None, 32, 1, None, 1) + (None,) * 5),
                       ("aog_telemetry_get_state", (None,) * 3), ("aog_telemetry_set_state", (None,) * 3)):
        assert getattr(lib, name)(*args) == -1 and name.encode() in lib.aog_last_error(), name
    assert lib.aog_telemetry_state_bytes(None) == 0
    lib.aog_telemetry_destroy(None)
    assert "telemetry" in __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"]).UNITS


@pytest.mark.parametrize("kw", [dict(batch=0), dict(act_dim=0), dict(act_dim=129), dict(length=32), dict(length=2048), dict(length=96)])
def test_create_refuses_bad_dimensions_before_any_device_work(kw):
    import ctypes as C

    cfg = dict(batch=2, act_dim=8, length=64, env_id_base=0)
    cfg.update(kw)
    h = C.c_void_p()
    lib = _lib.load()
    assert lib.aog_telemetry_create(C.byref(_lib.AogTelemetryConfig(*cfg.values())), 0, C.byref(h)) == -1 and not h.value
    assert b"aog_telemetry_create" in lib.aog_last_error()


def test_a_sinusoid_on_a_bin_stays_in_three_bins():
    S, k0 = 64, 5
    n = np.arange(4 * S)
    x = (3.0 * np.cos(2 * np.pi * k0 * n / S + 0.3))[:, None] + np.array([[0.0, 1e4]])
    phi, nseg = ref.welch_psd(x, S)
    assert nseg == 7
    for row, col in zip(phi, x.T):
        out = np.delete(row, [k0 - 1, k0, k0 + 1])
        # what rounding leaves elsewhere: |X_k| <= 8 S eps max|x| (the mean of the second mode is 3000 times its fluctuation), Phi < |X|^2
        print("largest Phi outside the three bins:", np.abs(out).max(), "of", row.max())
        assert np.abs(out).max() < (8 * S * np.finfo(float).eps * np.abs(col).max()) ** 2
        assert abs(row.sum() - 4.5) < 1e-9    # the variance of 3 cos


def test_white_noise_sums_to_its_variance():
    """sum_k Phi[k] estimates sigma^2 (1 - 1/S) (the segment mean takes one degree of freedom).  Its relative standard deviation: a Hann
    segment has (sum w^2)^2 / sum w^4 = 18 S / 35 equivalent degrees of freedom, half-overlapped segments count as nseg / 2 independent
    ones at the least, so std <= sqrt(2 / (18 S / 35 * nseg / 2)); the bound is 4 of them."""
    S, sigma = 64, 2.5
    x = sigma * np.random.RandomState(4).randn(S * 40, 6)
    phi, nseg = ref.welch_psd(x, S)
    assert nseg == 79
    tol = 4 * math.sqrt(2 / (18 * S / 35 * nseg / 2))
    got = phi.sum(axis=1) / (sigma ** 2 * (1 - 1 / S))
    print("sum Phi / variance:", got, "tolerance", tol)
    assert np.all(np.abs(got - 1) < tol)


def test_rejection_at_delay_1_is_the_closed_form():
    S = 128
    grid = np.array([0.05, 0.4, 1.3])
    z1 = np.exp(-2j * np.pi * np.arange(1, S // 2 + 1) / S)
    want = np.abs(1 - z1[None, :]) ** 2 / np.abs(1 - (1 - grid[:, None]) * z1[None, :]) ** 2
    np.testing.assert_allclose(ref.rejection(S, 1, grid), want, rtol=1e-11, atol=0)   # (1 - cos at k = 1 cancels 3 digits in both forms)
    np.testing.assert_allclose(ref.rejection(S, 1, grid, np.longdouble).astype(float), want, rtol=1e-11, atol=0)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_gain_limit_is_where_a_root_reaches_the_unit_circle(d):
    g_max = tel.gain_limit(d)
    for g, stable in ((g_max * (1 - 1e-6), True), (g_max * (1 + 1e-6), False)):
        poly = np.zeros(d + 1)
        poly[0] = 1.0
        poly[1] -= 1.0
        poly[-1] += g
        assert (np.abs(np.roots(poly)).max() < 1.0) == stable, (d, g)
    grid = tel.default_grid(d)
    assert len(grid) == 32 and np.all(np.diff(grid) > 0) and grid[0] > 0 and grid[-1] < g_max
    np.testing.assert_allclose([grid[0], grid[-1]], [0.02 * g_max, 0.8 * g_max], rtol=1e-12)
    assert tel.gain_limit(1) == 2.0 and abs(tel.gain_limit(2) - 1.0) < 1e-15


def test_a_slow_noisy_mode_gets_a_lower_gain_than_a_fast_clean_one():
    x = ref.ar1_modes(7, 2048, 2, pole=[0.999, 0.95], drive=[0.02, 1.0], noise=[1.0, 0.01])
    for d in (1, 2):
        gain, cost, J, _, nseg = ref.optimise(x, 128, d, tel.default_grid(d))
        print("delay", d, "gains", gain, "costs", cost)
        assert nseg == 31 and gain[0] < gain[1]
        assert np.all(cost == J.min(axis=1))


def test_the_ring_restatement_wraps_skips_and_masks():
    ring = ref.RingReference(3, 2, 8)
    for t in range(11):
        y = np.full((3, 2), float(t))
        if t == 4:
            y[1, 0] = np.inf
        ring.push(y, mask=[True, True, t % 2 == 0])
    assert list(ring.count) == [11, 10, 6] and list(ring.skipped) == [0, 1, 0]
    assert list(ring.series(0)[:, 0]) == [3, 4, 5, 6, 7, 8, 9, 10] and list(ring.series(1)[:, 0]) == [2, 3, 5, 6, 7, 8, 9, 10]
    assert list(ring.series(2)[:, 0]) == [0, 2, 4, 6, 8, 10]
    ring.reset([False, True, False])
    assert list(ring.count) == [11, 0, 6] and not ring.hist[1].any()


class _Env:
    num_envs, num_modes, wavelength_wfs, pyramid, SH_operation, max_steps, device = 2, 4, 1.5e-6, None, True, 3, "cpu"


def test_argument_errors_come_before_any_handle():
    t = tel.ModalTelemetry(2, 8, length=64)
    for seg in (48, 128, 16, 33.5):          # not a power of two, S > T, below 32
        with pytest.raises(ValueError, match="segment"):
            t.psd(segment=seg)
        with pytest.raises(ValueError, match="segment"):
            t.optimise_gains(segment=seg)
    for delay in (0, 5, 1.5):
        with pytest.raises(ValueError, match="delay"):
            t.optimise_gains(delay=delay)
        with pytest.raises(ValueError, match="delay"):
            tel.gain_limit(delay)
    for delay, g in ((1, 2.0), (2, 1.0), (2, 1.5), (1, 0.0), (1, -0.1), (1, float("nan"))):   # unstable, or not a gain
        with pytest.raises(ValueError, match="stable gains"):
            t.optimise_gains(delay=delay, grid=[0.1, g] if g > 0.1 else [g, 0.1])
    with pytest.raises(ValueError, match="ascending"):
        t.optimise_gains(grid=[0.5, 0.4, 0.3])
    with pytest.raises(ValueError, match="ascending"):
        t.optimise_gains(grid=[0.3, 0.3])
    with pytest.raises(ValueError, match="1 to 64"):
        t.optimise_gains(grid=np.linspace(0.01, 1.0, 65))
    with pytest.raises(ValueError, match="1 to 64"):
        t.optimise_gains(grid=[])
    assert t._handle is None
    with pytest.raises(ValueError, match="act_dim"):
        tel.ModalTelemetry(2, 129)
    with pytest.raises(ValueError, match="act_dim"):
        tel.ModalTelemetry(2, 0)
    for length in (32, 100, 2048):
        with pytest.raises(ValueError, match="length"):
            tel.ModalTelemetry(2, 8, length=length)
    with pytest.raises(ValueError, match="num_envs"):
        tel.ModalTelemetry(0, 8)


def test_integrator_and_rollout_argument_checks_need_no_device():
    from adaptive_optics_gym_amd import ModalIntegrator, ModalTelemetry
    from adaptive_optics_gym_amd.rollout import rollout

    assert ModalTelemetry is tel.ModalTelemetry
    with pytest.raises(ValueError, match="measurement"):
        ModalIntegrator(_Env(), measurement="shack")
    with pytest.raises(ValueError, match="pyramid=dict"):
        ModalIntegrator(_Env(), measurement="pyramid")
    with pytest.raises(ValueError, match="delay"):
        ModalIntegrator(_Env(), delay=0)
    with pytest.raises(ValueError, match="stable gains"):
        ModalIntegrator(_Env(), delay=2, gain=1.0)
    with pytest.raises(ValueError, match="leak"):
        ModalIntegrator(_Env(), leak=1.5)
    with pytest.raises(ValueError, match="telemetry holds"):
        ModalIntegrator(_Env(), telemetry=ModalTelemetry(3, 4))
    with pytest.raises(ValueError, match="controller=ModalIntegrator"):
        rollout(_Env(), None, policy="modal")
    with pytest.raises(ValueError, match="controller=ModalIntegrator"):
        rollout(_Env(), None, policy="ideal", controller=object())
    env = _Env()
    ctrl = ModalIntegrator(env, gain=0.3)
    assert ctrl.telemetry._handle is None and tuple(ctrl.gains.shape) == (2, 4) and float(ctrl.gains[1, 3]) == 0.3
    with pytest.raises(ValueError, match="another env"):
        rollout(_Env(), None, policy="modal", controller=ctrl)
