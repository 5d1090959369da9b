"""Modal disturbance, host side (no GPU): ``ar2_parameters``, the argument checks of ``disturbance.py``, the C-ABI surface of
include/aogym_disturbance.h and the self-consistency of the host restatement (tests/disturbance_reference.py) the GPU tests compare with."""
import ctypes
import os
import re

import numpy as np
import pytest

import disturbance_reference as ref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.disturbance import MAX_TERMS, ar2_parameters, named_shape, resolve_terms

DT = 1e-3
NEW_SYMBOLS = ("aog_disturbance_config_size", "aog_disturbance_create", "aog_disturbance_destroy", "aog_disturbance_set_params", "aog_disturbance_reset",
               "aog_disturbance_advance", "aog_disturbance_coefficients", "aog_disturbance_state_bytes", "aog_disturbance_get_state",
               "aog_disturbance_set_state", "aog_upload_disturbance_basis", "aog_install_layer_sum_disturbed")


@pytest.mark.parametrize("f0", [30.0, 120.0])
@pytest.mark.parametrize("zeta", [0.01, 0.1])
@pytest.mark.parametrize("rms", [1.0, 3e-8])
def test_stationary_variance_is_rms_squared(f0, zeta, rms):
    """Independently of the closed form for b: the 2 x 2 Yule-Walker system of the recursion gives gamma_0 = rms^2 to 1e-12, and
    gamma_1 / gamma_0 is the rho1 the stationary start uses."""
    p = ar2_parameters(f0, zeta, rms, DT)
    var = ref.ar2_variance(p["a1"], p["a2"], p["b"])
    assert abs(var - rms * rms) <= 1e-12 * rms * rms
    assert p["sigma"] == rms and abs(p["rho1"] - p["a1"] / (1.0 - p["a2"])) <= 1e-15 and abs(p["rho1"]) < 1


@pytest.mark.parametrize("f0", [30.0, 120.0])
@pytest.mark.parametrize("zeta", [0.01, 0.1])
def test_spectrum_peaks_in_the_bin_nearest_f0(f0, zeta):
    p = ar2_parameters(f0, zeta, 1.0, DT)
    S = 512
    freqs = np.arange(S // 2 + 1) / (S * DT)
    spec = ref.ar2_spectrum(p["a1"], p["a2"], p["b"], freqs, DT)
    assert int(np.argmax(spec)) == int(np.argmin(np.abs(freqs - f0)))


def test_zero_rms_is_a_static_term():
    p = ar2_parameters(50.0, 0.05, 0.0, DT)
    assert p["b"] == 0.0 and p["sigma"] == 0.0
    out = resolve_terms(2, [dict(term=1, frequency=50.0, damping=0.05, rms=0.0)], [1e-8, -2e-8], DT, 3, 3, 0)
    assert out["offset"].shape == (3, 2) and np.all(out["offset"] == [1e-8, -2e-8]) and not out["b"].any() and not out["a1"][:, 0].any()


@pytest.mark.parametrize("kw", [dict(damping=0.0), dict(damping=1.0), dict(damping=-0.1), dict(frequency=0.0), dict(frequency=500.0), dict(frequency=-3.0),
                                dict(rms=-1e-9), dict(rms=float("nan")), dict(delta_t=0.0)])
def test_ar2_refusals(kw):
    args = dict(frequency=30.0, damping=0.02, rms=1e-8, delta_t=DT)
    args.update(kw)
    with pytest.raises(ValueError):
        ar2_parameters(**args)


def test_term_and_shape_refusals():
    vib = dict(term=0, frequency=30.0, damping=0.02, rms=1e-8)
    for bad in ([dict(vib, term=2)], [vib, vib], [dict(term=0, frequency=30.0)], [dict(vib, extra=1)], [dict(vib, rms=[1e-8, 2e-8])]):
        with pytest.raises(ValueError):
            resolve_terms(2, bad, None, DT, 3, 3, 0)
    with pytest.raises(ValueError, match="static"):
        resolve_terms(2, [], [1.0, 2.0, 3.0], DT, 3, 3, 0)
    # per-env values, and total_envs values sliced at the offset
    out = resolve_terms(1, [dict(vib, rms=[1e-8, 2e-8, 3e-8, 4e-8])], None, DT, 2, 4, 2)
    np.testing.assert_array_equal(out["sigma"][:, 0], [3e-8, 4e-8])
    x = np.linspace(-1, 1, 40)
    xx, yy = np.meshgrid(x, x)
    keep = (xx ** 2 + yy ** 2 <= 1).ravel()
    for name in ("tip", "tilt", "focus"):
        v = named_shape(name, xx.ravel()[keep], yy.ravel()[keep])
        assert abs(v.mean()) < 1e-14 and abs(np.sqrt(np.mean(v * v)) - 1.0) < 1e-14
    with pytest.raises(ValueError):
        named_shape("coma", xx.ravel(), yy.ravel())
    assert MAX_TERMS == 8


def test_cabi_surface_of_the_new_header(repo_root):
    """Declared in include/aogym_disturbance.h, bound, exported; null arguments return AOG_ERR_INVALID naming the entry point; the ABI
    version and aogym.h's own symbol set are untouched."""
    header = open(os.path.join(repo_root, "include", "aogym_disturbance.h")).read()
    main = open(os.path.join(repo_root, "include", "aogym.h")).read()
    lib = _lib.load()
    assert '#include "aogym.h"' in header
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(NEW_SYMBOLS) == set(_lib.DISTURBANCE_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name not in _lib.SYMBOLS and not re.search(r"\b%s\s*\(" % name, main), name
    assert lib.aog_abi_version() == _lib.ABI_VERSION == 22
    assert lib.aog_disturbance_config_size() == ctypes.sizeof(_lib.AogDisturbanceConfig) == 24
    null = None
    calls = {"aog_disturbance_create": (null, 0, null), "aog_disturbance_set_params": (null,) * 7, "aog_disturbance_reset": (null,) * 4,
             "aog_disturbance_advance": (null,) * 5, "aog_disturbance_coefficients": (null,) * 3, "aog_disturbance_get_state": (null,) * 3,
             "aog_disturbance_set_state": (null,) * 3, "aog_upload_disturbance_basis": (null, null, 1),
             "aog_install_layer_sum_disturbed": (null, null, 1, null, 1, null)}
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1 and name.encode() in lib.aog_last_error(), name
    assert lib.aog_disturbance_state_bytes(None) == 0
    lib.aog_disturbance_destroy(None)
    # the config's own checks need no device either
    out = ctypes.c_void_p()
    for cfg, word in ((_lib.AogDisturbanceConfig(21, 4, 2, 0, 1), b"abi_version"), (_lib.AogDisturbanceConfig(22, 0, 2, 0, 1), b"num_envs"),
                      (_lib.AogDisturbanceConfig(22, 4, 0, 0, 1), b"n_terms"), (_lib.AogDisturbanceConfig(22, 4, 9, 0, 1), b"n_terms")):
        assert lib.aog_disturbance_create(ctypes.byref(cfg), 0, ctypes.byref(out)) == -1 and word in lib.aog_last_error()
    build = __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"])
    assert "disturbance" in build.UNITS and any(p.endswith("aogym_disturbance.h") for p in build.source_files())


def test_host_restatement_of_the_generator():
    """The restatement against a scalar loop of the header's formulas, masks included; a long run has the stationary variance."""
    rng = np.random.RandomState(3)
    B, K = 4, 2
    p = ar2_parameters(40.0, 0.05, 2.0, DT)
    params = {k: np.full((B, K), p[k]) for k in ("a1", "a2", "b", "sigma", "rho1")}
    params["offset"] = rng.randn(B, K)
    g = ref.Generator(params)
    n = rng.randn(B, K, 2)
    g.reset(n)
    assert g.counter == 1
    np.testing.assert_array_equal(g.x_prev, p["sigma"] * n[..., 0])
    np.testing.assert_array_equal(g.x, p["sigma"] * (p["rho1"] * n[..., 0] + np.sqrt(1 - p["rho1"] * p["rho1"]) * n[..., 1]))
    mask = np.array([True, False, True, True])
    x0, xp0 = g.x.copy(), g.x_prev.copy()
    n = rng.randn(B, K)
    c = g.advance(n, mask)
    for b in range(B):
        for k in range(K):
            if mask[b]:
                want = (p["a1"] * x0[b, k] + p["a2"] * xp0[b, k]) + p["b"] * n[b, k]
                assert g.x[b, k] == want and g.x_prev[b, k] == x0[b, k] and c[b, k] == params["offset"][b, k] + want
            else:
                assert g.x[b, k] == x0[b, k] and g.x_prev[b, k] == xp0[b, k] and c[b, k] == params["offset"][b, k] + x0[b, k]
    assert g.blob().size == 16 * B * K + 8 and g.counter == 2
    big = ref.Generator({k: np.full((256, 1), p[k]) for k in ("a1", "a2", "b", "sigma", "rho1")} | {"offset": np.zeros((256, 1))})
    big.reset(rng.randn(256, 1, 2))
    xs = np.stack([big.advance(rng.randn(256, 1)).copy() for _ in range(2000)])
    assert abs(xs.var() / 4.0 - 1.0) < 0.1


def test_host_restatement_of_the_disturbed_sum():
    import layered_reference as lref

    rng = np.random.RandomState(5)
    N, B, K = 12, 5, 3
    yy, xx = np.mgrid[:N, :N]
    ap = np.flatnonzero(((yy - 5.5) ** 2 + (xx - 5.5) ** 2 <= 36).ravel()).astype(np.int32)
    masters = [rng.randn(B, N, N) * 1e-6 for _ in range(2)]
    origins = [rng.randint(0, N, size=(B, 2)) for _ in range(2)]
    basis, coeff = rng.randn(K, ap.size), rng.randn(B, K) * 1e-7
    plain = lref.install(masters, origins, ap, N, 1.5e-6)
    zero = ref.install(masters, origins, ap, N, 1.5e-6, np.zeros((B, K)), basis)
    np.testing.assert_array_equal(zero["s"], plain["s"])
    # (the mean is summed in the kernel's fixed order here and by numpy's pairwise sum there: equal to that freedom)
    bound = ap.size * 2.0 ** -53 * np.abs(plain["s"]).max()
    assert np.abs(zero["mean"] - plain["mean"]).max() <= bound and np.abs(zero["psi64"] - plain["psi64"]).max() <= bound
    wide = rng.randn(3, 700)
    assert np.abs(ref.mean_in_fixed_order(wide) - wide.mean(axis=1)).max() <= 700 * 2.0 ** -53 * np.abs(wide).max()
    np.testing.assert_array_equal(ref.mean_in_fixed_order(np.ones((2, 300)) * 0.5), [0.5, 0.5])
    out = ref.install(masters, origins, ap, N, 1.5e-6, coeff, basis)
    np.testing.assert_allclose(out["s"] - plain["s"], coeff @ basis, rtol=0, atol=1e-20)
    # term order matters only in the last bits, and a piston shape changes nothing but the mean
    piston = ref.install(masters, origins, ap, N, 1.5e-6, coeff[:, :1], np.ones((1, ap.size)))
    np.testing.assert_allclose(piston["psi64"], plain["psi64"], rtol=0, atol=1e-20)
