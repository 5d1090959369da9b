"""Layer altitudes and sightlines, host side (no GPU): the geometry helpers of ``layered.py`` (default meta-pupil, shift formula and sign,
margin checks), the validation that runs before anything is created, the C-ABI surface of include/aogym_sightline.h, the stream-coverage
rule for that header and the self-consistency of the host restatement (tests/sightline_reference.py) the GPU tests compare with."""
import ast
import os
import re

import numpy as np
import pytest

import layered_reference as lref
import sightline_reference as ref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd import layered as L
from test_stream_coverage_cpu import ROOT, _python_callers, stream_entry_points

NEW_SYMBOLS = ("aog_install_layer_sum_sightline",)
PITCH = 0.5 / 32


# ---- the default meta-pupil ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,theta,N,want_c,want_n", [
    ([0.0, 1e4], (1e-5, 0.0), 32, 8, 48),         # 6.4 pixels: ceil = 7, + 1 = 8; 32 + 16 = 48 is a multiple of 4
    ([0.0, 8192.0], (0.0, -2.0 ** -17), 32, 5, 44),   # exactly 4 pixels (powers of two; the sign does not matter): 4 + 1 = 5; 42 rounds up to 44
    ([0.0, 5e3, 1e4], (3e-6, 4e-6), 32, 4, 40),   # the highest layer and the larger component decide: 2.56 -> 3 + 1
    ([0.0, 0.0], (1e-3, 1e-3), 32, 1, 36),        # nothing above the ground: the formula's 0 + 1
    ([1e4], (1e-5, 0.0), 30, 8, 46),              # N no multiple of 4: N + 2 c as it is
])
def test_default_meta_pupil_rule(h, theta, N, want_c, want_n):
    angle = L.resolve_field_angle(theta, 3)
    c = L.required_margin(np.array(h), [np.zeros((3, 2)), angle], 0.5 / 32)
    assert c == want_c
    n = L.default_meta_pupil_pixels(N, c)
    assert n == want_n and (n - N) % 2 == 0 and (n - N) // 2 >= c
    # the smallest: one accepted size less leaves less than the margin
    step = 4 if N % 4 == 0 else 2
    assert (n - step - N) // 2 < c


def test_the_margin_covers_every_declared_sightline():
    h = np.array([0.0, 1e4])
    angles = [L.resolve_field_angle(a, 2) for a in ((0.0, 0.0), (2e-6, 0.0), (0.0, -9e-6))]
    assert L.required_margin(h, angles, PITCH) == int(np.ceil(9e-6 * 1e4 / PITCH)) + 1 == 7
    margins = np.array([0, 7])
    for a in angles:
        L.check_margin(L.sightline_shifts(h, a, PITCH), margins, "angle")
    with pytest.raises(ValueError, match="layer 1 .* leaves 6"):
        L.check_margin(L.sightline_shifts(h, L.resolve_field_angle((0.0, 1e-5), 2), PITCH), margins, "angle")
    # a ground layer takes no shift at all, and no margin: only an altitude of exactly 0 passes c = 0
    L.check_margin(L.sightline_shifts(np.array([0.0]), angles[2], PITCH), [0], "ground")
    with pytest.raises(ValueError, match="layer 0"):
        L.check_margin(L.sightline_shifts(np.array([1.0]), angles[2], PITCH), [0], "ground")


# ---- the shift formula and its sign ----------------------------------------------------------------------------------------------------------
def test_shift_formula_and_sign():
    h = np.array([0.0, 2e3, 1e4])
    angle = np.array([[1e-5, -2e-5], [0.0, 3e-6]])
    s = L.sightline_shifts(h, angle, PITCH)
    assert s.shape == (3, 2, 2) and s.dtype == np.float64 and s.flags.c_contiguous
    for l in range(3):
        for b in range(2):
            for j in range(2):
                assert s[l, b, j] == (h[l] * angle[b, j]) / PITCH      # the product, then the quotient
    assert not s[0].any() and s[2, 0, 0] > 0 > s[2, 0, 1]
    # the sign, through the restatement: a front that looks along +theta_x reads the layer further along +x — the value at front pixel
    # (iy, ix) is the layer's at (iy + c, ix + c + 3)
    N, n = 8, 16
    c = (n - N) // 2
    screen = np.arange(n * n, dtype=np.float64).reshape(1, n, n)
    ap = np.arange(N * N)
    pitch = 0.5 / N
    shift = L.sightline_shifts(np.array([1e4]), np.array([[3 * pitch / 1e4, 0.0]]), pitch)
    got = ref.displaced_layer(screen[:1], shift[0], ap, N).reshape(N, N)
    np.testing.assert_allclose(shift[0], [[3.0, 0.0]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, screen[0, c:c + N, c + 3:c + 3 + N], rtol=0, atol=1e-9)


def test_field_angle_forms():
    one = L.resolve_field_angle((1e-6, -2e-6), 3)
    np.testing.assert_array_equal(one, [[1e-6, -2e-6]] * 3)
    assert not L.resolve_field_angle(None, 4).any()
    per_env = np.arange(10.0).reshape(5, 2) * 1e-6
    np.testing.assert_array_equal(L.resolve_field_angle(per_env[:3], 3, 5, 0), per_env[:3])
    np.testing.assert_array_equal(L.resolve_field_angle(per_env, 3, 5, 2), per_env[2:])      # total_envs values, sliced at the offset
    for bad in ((1e-6,), np.zeros((3, 3)), np.zeros((4, 2)), (np.nan, 0.0), np.zeros((2, 3, 2))):
        with pytest.raises(ValueError):
            L.resolve_field_angle(bad, 3, 5, 0)


# ---- validation before anything is created ---------------------------------------------------------------------------------------------------
LAYERS = [{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}]


@pytest.mark.parametrize("kw,word", [
    (dict(layer_altitudes=[0.0]), "one altitude in metres per layer"),
    (dict(layer_altitudes=[0.0, -1.0]), ">= 0"),
    (dict(layer_altitudes=[0.0, np.inf]), "finite"),
    (dict(layer_altitudes=[[0.0, 1.0]]), "per layer"),
    (dict(field_angle=(1e-6, 0.0)), "need layer_altitudes"),
    (dict(meta_pupil_pixels=48), "need layer_altitudes"),
    (dict(sightlines={"uplink": (1e-6, 0.0)}), "need layer_altitudes"),
    (dict(layer_altitudes=[0.0, 1e4], field_angle=(1e-6,)), "field_angle"),
    (dict(layer_altitudes=[0.0, 1e4], field_angle=(np.nan, 0.0)), "field_angle"),
    (dict(layer_altitudes=[0.0, 1e4], field_angle=np.zeros((3, 2))), "field_angle"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=47), "even difference"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=30), "even difference"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=40.5), "even difference"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=40, field_angle=(1e-5, 0.0)), "leaves 3"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=40, sightlines={"uplink": (0.0, 1e-5)}), "sightline 'uplink'"),
    (dict(layer_altitudes=[0.0, 1e4], sightlines=[(0.0, 1e-5)]), "dict"),
])
def test_geometry_is_refused_before_anything_is_created(kw, word, monkeypatch):
    """Every one of these raises ValueError out of the constructor's own checks: the base constructor (which loads the library and asks
    for a device) is never reached."""
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    def never(self, *a, **k):
        raise AssertionError("the env was being created")

    monkeypatch.setattr(BatchedAOEnv, "__init__", never)
    with pytest.raises(ValueError, match=word):
        LayeredAOEnv(2, "cuda:0", atm_layers=LAYERS, atm_fried=0.15, act_type="zernike", act_dim=6, num_pupil_pixels=32, verbose=False, **kw)


def test_resolve_layers_is_unchanged():
    """``layer_altitudes`` is a keyword of its own: a layer dict takes exactly 'fraction' and 'speed', as before."""
    plan = L.resolve_layers(LAYERS, 0.15, 3)
    assert [sorted(p) for p in plan] == [["fraction", "fried", "speed"]] * 2
    assert plan[0]["fried"] == 0.15 * 0.6 ** (-3.0 / 5.0) and plan[1]["speed"] == 50.0
    with pytest.raises(ValueError, match="exactly the keys"):
        L.resolve_layers([dict(LAYERS[0], altitude=0.0), LAYERS[1]], 0.15, 3)
    with pytest.raises(ValueError, match="sum to 1"):
        L.resolve_layers([LAYERS[0]], 0.15, 3)
    assert L.resolve_altitudes(None, 2) is None
    np.testing.assert_array_equal(L.resolve_altitudes((0, 1e4), 2), [0.0, 1e4])


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def _header(repo_root=ROOT):
    with open(os.path.join(repo_root, "include", "aogym_sightline.h")) as f:
        return f.read()


def test_cabi_surface_of_the_new_header(repo_root):
    """Declared in include/aogym_sightline.h, bound, exported by the built library; null arguments return AOG_ERR_INVALID naming the entry
    point; the ABI version and the other headers' symbol sets are untouched."""
    header = _header(repo_root)
    lib = _lib.load()
    assert '#include "aogym.h"' in header
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(NEW_SYMBOLS) == set(_lib.SIGHTLINE_SYMBOLS)
    for other in ("aogym.h", "aogym_disturbance.h"):
        text = open(os.path.join(repo_root, "include", other)).read()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name) and name not in _lib.SYMBOLS and name not in _lib.DISTURBANCE_SYMBOLS and not re.search(r"\b%s\s*\(" % name, text)
    assert lib.aog_abi_version() == _lib.ABI_VERSION == 22
    for args in ((None, None, 1, None, None, 0, None),):
        assert lib.aog_install_layer_sum_sightline(*args) == -1 and b"aog_install_layer_sum_sightline" in lib.aog_last_error()
    build = __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"])
    assert any(p.endswith("aogym_sightline.h") for p in build.source_files())
    assert any(p.endswith("aogym_sightline.h") for p in build._unit_deps("layers"))


def test_the_header_states_the_arithmetic():
    text = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    for phrase in ("v_l = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))", "never a fused multiply-add", "modulo N_l", "c_l - 1",
                   "y0 = floor(sy)"):
        assert phrase in text, phrase


def test_the_stream_entry_point_is_placed():
    """The rule of test_stream_coverage_cpu.py for this header: its one entry point with a ``void* stream`` is driven on a caller's side
    stream by the test that ``COVERED`` of test_gpu_sightline.py names, and a public Python function calls it."""
    assert stream_entry_points(_header()) == ["aog_install_layer_sum_sightline"]
    with open(os.path.join(ROOT, "tests", "test_gpu_sightline.py")) as f:
        tree = ast.parse(f.read())
    covered = next(ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "COVERED")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert set(covered) == set(stream_entry_points(_header())) and set(covered.values()) <= tests
    assert "layered.py" in _python_callers("aog_install_layer_sum_sightline")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_host_restatement_of_the_displaced_sum():
    rng = np.random.RandomState(7)
    N, n, B = 12, 20, 3
    c = (n - N) // 2
    yy, xx = np.mgrid[:N, :N]
    ap = np.flatnonzero(((yy - 5.5) ** 2 + (xx - 5.5) ** 2 <= 36).ravel()).astype(np.int32)
    iy, ix = np.divmod(ap, N)
    ground, high = rng.randn(B, N, N) * 1e-6, rng.randn(B, n, n) * 1e-6
    zero = np.zeros((B, 2))
    # zero shifts: the centre of the meta-pupil, exactly; with N_l = N the plain layer sum, exactly
    np.testing.assert_array_equal(ref.displaced_layer(high, zero, ap, N), high[:, c:c + N, c:c + N].reshape(B, -1)[:, ap])
    np.testing.assert_array_equal(ref.sightline_sum([ground, ground[::-1]], [zero, zero], ap, N),
                                  lref.layer_sum([ground, ground[::-1]], [zero.astype(int)] * 2, ap, N))
    # whole-pixel shifts of both signs, up to c - 1: translations, exactly
    shift = np.array([[3.0, -2.0], [-(c - 1.0), c - 1.0], [0.0, 1.0]])
    got = ref.displaced_layer(high, shift, ap, N)
    for b in range(B):
        sx, sy = int(shift[b, 0]), int(shift[b, 1])
        np.testing.assert_array_equal(got[b], high[b, iy + c + sy, ix + c + sx])
    # fractional shifts: a scalar loop of the header's formula, bracket by bracket
    shift = np.array([[0.25, -0.5], [-2.75, 1.125], [c - 1.0, -(c - 1.0) + 0.3]])
    got = ref.displaced_layer(high, shift, ap, N)
    for b in range(B):
        sx, sy = shift[b]
        x0, y0 = int(np.floor(sx)), int(np.floor(sy))
        fx, fy = sx - x0, sy - y0
        gx, gy = 1.0 - fx, 1.0 - fy
        for j in (0, ap.size // 2, ap.size - 1):
            y, x = iy[j] + c + y0, ix[j] + c + x0
            assert 0 <= y and y + 1 < n and 0 <= x and x + 1 < n      # inside the margin nothing wraps
            v = (gy * ((gx * high[b, y, x]) + (fx * high[b, y, x + 1]))) + (fy * ((gx * high[b, y + 1, x]) + (fx * high[b, y + 1, x + 1])))
            assert got[b, j] == v
    # a linear ramp is reproduced by the bilinear read (to rounding), whatever the fraction
    ramp = np.broadcast_to((2.0 * np.arange(n)[:, None] - 3.0 * np.arange(n)[None, :]) * 1e-7, (B, n, n))
    want = (2.0 * (iy + c + shift[:, 1:2]) - 3.0 * (ix + c + shift[:, 0:1])) * 1e-7
    np.testing.assert_allclose(ref.displaced_layer(ramp, shift, ap, N), want, rtol=0, atol=1e-18)
    # install: the terms and the mean as the disturbed form's
    basis, coeff = rng.randn(2, ap.size), rng.randn(B, 2) * 1e-7
    out = ref.install([ground, high], [zero, shift], ap, N, 1.5e-6, coeff, basis)
    plain = ref.install([ground, high], [zero, shift], ap, N, 1.5e-6)
    np.testing.assert_allclose(out["s"] - plain["s"], coeff @ basis, rtol=0, atol=1e-20)
    assert np.abs(out["psi64"].mean(axis=1)).max() < 1e-20 and out["tiles"].dtype == np.float32
