"""CPU tests of the science camera's host side: its tables against the oracle's science-arm propagation, the C-ABI surface and the
argument refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from adaptive_optics_gym_amd import _lib, optics_host
from adaptive_optics_gym_amd.params import OpticalParams
from helpers import smooth_screens
from oracle.ao_env_oracle import AOEnvOracle

N, A = 64, 16
SYMBOLS = ("aog_upload_science", "aog_science_integrate", "aog_science_clear", "aog_science_read")


@pytest.fixture(scope="module")
def aberrated():
    """One aberrated oracle state (screen + mirror), its science-arm image under the camera's normalisation, and phi_sci on the pupil grid."""
    psi = smooth_screens(1, N, 3)[0]
    env = AOEnvOracle(act_dim=A, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=N, screen=psi.ravel(), verbose=False)
    env.reset()
    env.step(np.random.RandomState(4).randn(A).astype(np.float32))
    image = (env.wf_sci_focal_plane.power / (env.unaberrated_PSF.max() * env.wf_wfs.total_power)).reshape(240, 240)
    T = optics_host.build_tables(OpticalParams(num_pupil_pixels=N), "num_actuators", A, 2)
    theta = psi.ravel()[T.ap_index] + 4 * np.pi * (T.modes @ env.deformable_mirror.actuators)
    E = np.zeros(N * N, dtype=complex)
    E[T.ap_index] = np.exp(1j * theta / 2.2e-6)
    return env, image, E.reshape(N, N), T


@pytest.mark.parametrize("w", [240, 64, 48])
def test_window_tables_reproduce_the_oracle_image(aberrated, w):
    """|m1 E m2|^2 in numpy float64 == the window of wf_sci_focal_plane.power / (unaberrated_PSF.max() x total power), to 1e-10 of the
    peak (the bound of test_collapsed_tables_reproduce_literal_pipeline for the same kind of claim); the centre pixel is the oracle's
    Strehl ratio."""
    env, image, E, _ = aberrated
    t = optics_host.science_tables(OpticalParams(num_pupil_pixels=N), w)
    assert t.m1.shape == (w, N) and t.m2.shape == (N, w) and t.ee_bin.shape == (w, w) and t.ee_bin.dtype == np.int32
    got = np.abs(t.m1 @ E @ t.m2) ** 2
    lo = 120 - w // 2
    ref = image[lo:lo + w, lo:lo + w]
    assert np.abs(got - ref).max() <= 1e-10 * ref.max()
    np.testing.assert_allclose(got[w // 2, w // 2], env.last_strehl, rtol=1e-10)
    np.testing.assert_allclose(t.phase_ratio, 1.5e-6 / 2.2e-6, rtol=1e-15)


def test_flat_wavefront_gives_one_at_the_centre_and_peak_fraction_is_the_unaberrated_peak(aberrated):
    env, _, _, T = aberrated
    mask = np.zeros(N * N)
    mask[T.ap_index] = 1.0
    for w in (240, 64, 2):
        t = optics_host.science_tables(OpticalParams(num_pupil_pixels=N), w)
        # the on-axis kernel is exactly 1 / n_ap per aperture pixel; the sum of n_ap of them rounds once per term of the two products
        assert np.all(t.m1[w // 2] == 1.0 / T.n_ap) and np.all(t.m2[:, w // 2] == 1.0)
        flat = np.abs(t.m1 @ mask.reshape(N, N) @ t.m2) ** 2
        assert abs(flat[w // 2, w // 2] - 1.0) <= 4 * N * np.finfo(np.float64).eps
        assert flat.max() == flat[w // 2, w // 2]
        np.testing.assert_allclose(t.peak_fraction, env.unaberrated_PSF.max(), rtol=1e-12)   # (the oracle's beam has unit power there)


def test_encircled_energy_bins_and_radii():
    p = OpticalParams(num_pupil_pixels=N)
    t = optics_host.science_tables(p, 240)
    np.testing.assert_array_equal(t.radii, [1, 2, 3, 5, 8])
    i = np.arange(240) - 120
    r = np.hypot(i[:, None], i[None, :]) / p.focal_q
    for k, R in enumerate(t.radii):
        np.testing.assert_array_equal((t.ee_bin >= 0) & (t.ee_bin <= k), r <= R * (1 + 1e-9))
    assert t.ee_bin[120, 120] == 0 and t.ee_bin[120, 124] == 0 and t.ee_bin[120, 125] == 1 and t.ee_bin[0, 0] == -1
    # clipped to the largest circle the window holds whole, duplicates dropped
    np.testing.assert_array_equal(optics_host.science_tables(p, 48).radii, [1, 2, 3, 5, 5.75])
    np.testing.assert_array_equal(optics_host.science_tables(p, 8).radii, [0.75])
    t = optics_host.science_tables(p, 64, radii=[0.5, 4.0])
    assert t.radii.tolist() == [0.5, 4.0] and t.ee_bin.max() == 1 and (t.ee_bin == 0).sum() == 13


@pytest.mark.parametrize("window", [63, 0, 1, -2, 242, 64.5])
def test_bad_windows_raise(window):
    with pytest.raises(ValueError, match="science_window"):
        optics_host.science_tables(OpticalParams(num_pupil_pixels=N), window)


@pytest.mark.parametrize("radii", [[], [2.0, 1.0], [1.0, 1.0], [-1.0], [1.0, 8.0], list(np.arange(1, 34) * 0.1)])
def test_bad_radii_raise(radii):
    with pytest.raises(ValueError, match="science_radii"):
        optics_host.science_tables(OpticalParams(num_pupil_pixels=N), 64, radii=radii)   # (window 64 holds radii up to 7.75)


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_unchanged(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 22 and lib.aog_abi_version() == 22 and re.search(r"#define AOG_ABI_VERSION\s+22\b", header)
    assert lib.aog_struct_size(9) == -1   # no struct was added: the entry points take pointers and scalars only


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    m = np.zeros(8)
    b = np.zeros(4, dtype=np.int32)
    p = ctypes.c_void_p
    assert lib.aog_upload_science(None, p(m.ctypes.data), p(m.ctypes.data), 2, 0.68, 0.05, p(b.ctypes.data), 1) == -1   # AOG_ERR_INVALID
    assert b"null argument" in lib.aog_last_error()
    assert lib.aog_science_integrate(None, None, None) == -1
    assert lib.aog_science_clear(None, None, None) == -1
    assert lib.aog_science_read(None, 0, 1, None, None, None, None, None) == -1
    assert b"aog_science_read" in lib.aog_last_error()
