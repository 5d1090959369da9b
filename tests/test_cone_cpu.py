"""Finite-range sources, host side (no GPU): the geometry helpers of ``layered`` (``cone_geometry``, the cone-aware margins, the default
meta-pupil), construction-time refusals and the state's range record, the C-ABI surface of include/aogym_cone.h (every refusal comes
before any device work — that this file passes without a GPU is the demonstration), the stream-coverage rule for the new header against
the tables of tests/test_gpu_cone.py, the self-consistency of the host restatement (tests/cone_reference.py), ``displaced_basis`` with a
magnification against it, and ``tilt_blind`` on a CPU solve of the normal equations."""
import ast
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import cone_reference as ref
import sightline_reference as sref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd import layered as L
from adaptive_optics_gym_amd import tomography as tm
from test_stream_coverage_cpu import ROOT, _python_callers, stream_entry_points

INVALID = -1
NEW_SYMBOLS = ("aog_install_layer_sum_cone", "aog_cone_check_geometry")
PITCH = 0.5 / 32


def _header():
    with open(os.path.join(ROOT, "include", "aogym_cone.h")) as f:
        return f.read()


# ---- the geometry ------------------------------------------------------------------------------------------------------------------------------
def test_cone_geometry_values():
    h = np.array([0.0, 1e4, 1.5e4])
    angle = L.resolve_field_angle([(5e-6, -2e-6), (0.0, 1e-6), (3e-6, 3e-6)], 3)
    H = np.array([9e4, np.inf, 2e4])
    g = L.cone_geometry(h, angle, H, PITCH)
    assert g.shape == (3, 3, 3) and g.dtype == np.float64 and g.flags.c_contiguous
    np.testing.assert_array_equal(g[:, :, :2], L.sightline_shifts(h, angle, PITCH))      # the shift is the sightline helper's
    assert np.all(g[0, :, 2] == 1.0)                                                     # h = 0: exactly 1
    assert np.all(g[:, 1, 2] == 1.0)                                                     # H = inf: exactly 1
    for l in (1, 2):
        for b in (0, 2):
            assert g[l, b, 2] == 1.0 - (h[l] / H[b])                                     # one rounded quotient, one rounded difference
    assert g[2, 2, 2] == 0.25 and g[1, 0, 2] == 1.0 - 1e4 / 9e4
    # a scalar range serves every env; None resolves to a plane wave
    np.testing.assert_array_equal(L.cone_geometry(h, angle, 9e4, PITCH)[:, :, 2], np.tile((1.0 - h / 9e4)[:, None], (1, 3)))
    assert np.all(np.isinf(L.resolve_range(None, 4))) and np.all(L.resolve_range(9e4, 4) == 9e4)
    np.testing.assert_array_equal(L.resolve_range([1e4, np.inf, 2e4, 3e4], 2, 4, 1), [np.inf, 2e4])      # global env ids, sliced
    for bad in (0.0, -1.0, float("nan"), [1e4, -2.0]):
        with pytest.raises(ValueError, match="range"):
            L.resolve_range(bad, 2)


def test_a_source_at_or_below_a_layer_is_refused_naming_it():
    angle = np.zeros((2, 2))
    with pytest.raises(ValueError, match="layer 1 at 10000 m lies at or above the source at 10000 m"):
        L.cone_geometry(np.array([0.0, 1e4]), angle, 1e4, PITCH)
    with pytest.raises(ValueError, match=r"mirror 0 at 20000 m .* 15000 m \(env 1\)"):
        L.cone_geometry(np.array([0.0, 1e4, 2e4]), angle, np.array([np.inf, 1.5e4]), PITCH, first_mirror=2)
    L.cone_geometry(np.array([0.0, 1e4]), angle, np.nextafter(1e4, 2e4), PITCH)      # just above: m > 0


def test_the_margin_arithmetic():
    """|s| + (1 - m) (N - 1) / 2 against c - 1: N = 32 (ctr = 15.5), a layer at 1e4 m read 3.2 pixels off, from 9e4 m: m = 8 / 9,
    (1 - m) ctr = 1.7222, reach 4.9222: c = 6 (the plane wave asks for 5)."""
    h = np.array([0.0, 1e4])
    angle = L.resolve_field_angle((5e-6, 0.0), 2)
    far, near = L.resolve_range(None, 2), L.resolve_range(9e4, 2)
    g = L.cone_geometry(h, angle, near, PITCH)
    reach = L.cone_reach(g, 32)
    assert reach[0] == 0.0 and reach[1] == abs(g[1, 0, 0]) + ((1.0 - g[1, 0, 2]) * 15.5) and abs(reach[1] - (3.2 + 15.5 / 9)) < 1e-12
    assert L.required_margin(h, [angle], PITCH) == 5
    assert L.required_margin_cone(h, [(angle, far)], PITCH, 32) == 5       # every range infinite: required_margin
    assert L.required_margin_cone(h, [(angle, near)], PITCH, 32) == 6
    assert L.required_margin_cone(h, [(angle, far), (np.zeros((2, 2)), L.resolve_range(2e4, 2))], PITCH, 32) == int(np.ceil(15.5 / 2)) + 1 == 9
    L.check_margin_cone(g, [0, 6], 32, "look")
    with pytest.raises(ValueError, match=r"look: layer 1 would be read 4\.922 pixels off the pupil .* leaves 4 \(margin c = 5"):
        L.check_margin_cone(g, [0, 5], 32, "look")
    with pytest.raises(ValueError, match="look: mirror 0 "):
        L.check_margin_cone(g, [0, 5], 32, "look", first_mirror=1)
    # the ground: no shift and m = 1 pass a margin of 0, anything else does not
    L.check_margin_cone(np.array([[[0.0, 0.0, 1.0]]]), [0], 32, "ground")
    for bad in ([0.25, 0.0, 1.0], [0.0, 0.0, 0.999]):
        with pytest.raises(ValueError, match="ground: layer 0"):
            L.check_margin_cone(np.array([[bad]]), [0], 32, "ground")
    for bad in ([0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [np.nan, 0.0, 1.0]):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            L.check_margin_cone(np.array([[bad]]), [8], 32, "m")
    # the restatement's check is the same rule
    assert ref.check(g, [32, 44], 32) and not ref.check(g, [32, 42], 32)
    # the existing helpers keep their results
    assert L.default_meta_pupil_pixels(32, 5) == 44 and L.default_meta_pupil_pixels(32, 6) == 44 and L.default_meta_pupil_pixels(32, 9) == 52


def test_the_default_margin_does_not_depend_on_the_part_of_the_batch():
    """The margin is sized for every declared range: a part that holds only plane-wave envs gets the whole batch's meta-pupil."""
    h = np.array([0.0, 1e4])
    stated = L.declared_range([9e4, np.inf, 2e4])
    whole = L.required_margin_cone(h, [(L.resolve_field_angle((5e-6, 0.0), 3), stated)], PITCH, 32)
    part = L.required_margin_cone(h, [(L.resolve_field_angle((5e-6, 0.0), 1), stated)], PITCH, 32)
    assert whole == part == int(np.ceil(3.2 + 7.75)) + 1
    np.testing.assert_array_equal(L.declared_range(None), [np.inf]), np.testing.assert_array_equal(L.declared_range(9e4), [9e4])
    with pytest.raises(ValueError, match="layer 1 at 10000 m lies at or above"):
        L.required_margin_cone(h, [(np.zeros((1, 2)), np.array([np.inf, 5e3]))], PITCH, 32)


def test_default_meta_pupil_sizes():
    """The default meta-pupil counts (1 - m) ctr: on axis, a layer at 1e4 m under a beacon at 2e4 m shrinks to half — 7.75 pixels at N = 32."""
    h = np.array([0.0, 1e4])
    on_axis = np.zeros((2, 2))
    assert L.default_meta_pupil_pixels(32, L.required_margin(h, [on_axis], PITCH)) == 36
    assert L.default_meta_pupil_pixels(32, L.required_margin_cone(h, [(on_axis, L.resolve_range(2e4, 2))], PITCH, 32)) == 52
    assert L.default_meta_pupil_pixels(16, L.required_margin_cone(h, [(on_axis, L.resolve_range(8e4, 2))], 0.5 / 16, 16)) == 20


# ---- construction-time validation, before anything is created ---------------------------------------------------------------------------------
LAYERS = [{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}]


@pytest.mark.parametrize("kw,word", [
    (dict(source_range=9e4), "source_range needs layer_altitudes"),
    (dict(layer_altitudes=[0.0, 1e4], source_range=0.0), "source_range: a range is in metres"),
    (dict(layer_altitudes=[0.0, 1e4], source_range=float("nan")), "source_range: a range is in metres"),
    (dict(layer_altitudes=[0.0, 1e4], source_range=[9e4, 9e4, 9e4]), "source_range"),
    (dict(layer_altitudes=[0.0, 1e4], source_range=1e4), "field_angle: layer 1 at 10000 m lies at or above the source"),
    (dict(layer_altitudes=[0.0, 1e4], sightlines={"lgs": dict(angle=(0.0, 0.0), range=5e3)}), "sightline 'lgs': layer 1 at 10000 m lies at or above"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=2e4)], source_range=1.5e4), "field_angle: mirror 0 at 20000 m"),
    (dict(layer_altitudes=[0.0, 1e4], sightlines={"lgs": dict(angle=(0.0, 0.0), reach=9e4)}), "a dict with 'angle'"),
    (dict(layer_altitudes=[0.0, 1e4], sightlines={"lgs": dict(range=9e4)}), "a dict with 'angle'"),
    # 3.2 pixels pass c = 6 as a plane wave; from 9e4 m the footprint's far edge adds 1.72: 4.92 > 5 - ... c = 5 leaves 4
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=42, field_angle=(5e-6, 0.0), source_range=9e4), "field_angle: layer 1 would be read 4.922"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=42, sightlines={"lgs": dict(angle=(5e-6, 0.0), range=9e4)}), "sightline 'lgs': layer 1 .* leaves 4"),
])
def test_ranges_are_refused_before_anything_is_created(kw, word, monkeypatch):
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    def never(self, *a, **k):
        raise AssertionError("the env was being created")

    monkeypatch.setattr(BatchedAOEnv, "__init__", never)
    args = dict(atm_layers=LAYERS, atm_fried=0.15, act_type="zernike", act_dim=6, num_pupil_pixels=32, verbose=False)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        LayeredAOEnv(2, "cuda:0", **args)


# ---- state: the ranges are recorded, a mismatch is refused -------------------------------------------------------------------------------------
class _Bare(L.LayeredAOEnv):
    """A LayeredAOEnv with the geometry of one layer at 1e4 m under N = 32 / N_L = 48 and no device behind it: what get_state / set_state do
    with ranges before and after the parts that need a device."""

    def __init__(self, source_range=None, lgs_range=None):
        self.num_envs = self.total_envs = 2
        self.global_env_offset = 0
        self.num_pupil_pixels = 32
        self.params = types.SimpleNamespace(pupil_pixel=PITCH)
        self._layers, self._mirrors, self.disturbance = [None, None], [], None
        self._altitudes = self._seen_at = np.array([0.0, 1e4])
        self._seen_margins = np.array([0, 8])
        self.source_range = L.resolve_range(source_range, 2)
        self._look(*self._shifts_for((2e-6, 0.0), "field_angle", self.source_range))
        rng = L.resolve_range(lgs_range, 2)
        sl = L.Sightline(self, "lgs", None, None, rng)
        sl._look(*self._shifts_for((-3e-6, 1e-6), "sightline 'lgs'", rng))
        self._sightlines = {"lgs": sl}

    def ranges_of(self):
        """The ranges' part of get_state()."""
        state = {"sightlines": {name: {} for name in self._sightlines}}
        self._record_ranges(state)
        return state

    def __del__(self):
        pass


def test_state_round_trip_and_the_mismatch_refusal():
    # get_state records a range where there is one (_record_ranges, the lines get_state runs); a plane-wave env's state has the keys it had
    plane, cone = _Bare(), _Bare(source_range=[9e4, 8e4], lgs_range=9e4)
    assert plane._geometry is None and plane._sightlines["lgs"]._geometry is None
    assert cone._geometry.shape == (2, 2, 3) and cone._geometry[1, 1, 2] == 1.0 - 1e4 / 8e4
    assert plane.ranges_of() == {"sightlines": {"lgs": {}}}
    saved = cone.ranges_of()
    np.testing.assert_array_equal(saved["source_range"], [9e4, 8e4])
    np.testing.assert_array_equal(saved["sightlines"]["lgs"]["range"], [9e4, 9e4])

    def refused(env, ranges, word):
        state = {"layers": [None, None], "field_angle": np.zeros((2, 2)), "sightlines": {"lgs": dict(angle=np.zeros((2, 2)), **ranges["sightlines"]["lgs"])}}
        if "source_range" in ranges:
            state["source_range"] = ranges["source_range"]
        env._check_servo_state = lambda state: None
        with pytest.raises(ValueError, match=word):
            env.set_state(state)

    refused(plane, saved, "set_state: the state was saved with source_range = .9.*, this env was built with .inf, inf.")
    refused(cone, plane.ranges_of(), "set_state: the state was saved with source_range = .inf, inf., this env was built with .90000")
    refused(_Bare(source_range=[9e4, 8e4]), saved, "sightline 'lgs': range")
    refused(_Bare(source_range=[9e4, 7e4], lgs_range=9e4), saved, "source_range")


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def test_cabi_surface_of_the_new_header(repo_root):
    header = _header()
    lib = _lib.load()
    assert '#include "aogym_conjugate.h"' in header
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(NEW_SYMBOLS) == set(_lib.CONE_SYMBOLS)
    for other in ("aogym.h", "aogym_disturbance.h", "aogym_sightline.h", "aogym_servo.h", "aogym_conjugate.h", "aogym_tomography.h", "aogym_lqg.h"):
        text = open(os.path.join(repo_root, "include", other)).read()
        for name in NEW_SYMBOLS:
            assert not re.search(r"\b%s\s*\(" % name, text), (other, name)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert not any(name in table for table in (_lib.SYMBOLS, _lib.DISTURBANCE_SYMBOLS, _lib.SIGHTLINE_SYMBOLS, _lib.CONJUGATE_SYMBOLS)), name
    assert lib.aog_abi_version() == _lib.ABI_VERSION == 22
    build = __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"])
    assert set(build.EXTRA_HEADERS["aogym_cone.h"]) == {"layers"}
    assert any(p.endswith("aogym_cone.h") for p in build.source_files())
    deps = build._unit_deps("layers")
    assert any(p.endswith("aogym_cone.h") for p in deps) and any(p.endswith("k_cone.h") for p in deps)


def test_the_installation_refuses_null_arguments():
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    block = C.c_void_p(C.addressof(keep))
    handles = (C.c_void_p * 1)(block.value)
    for args in ((None, None, 1, None, 0, None, None, 0, None), (None, handles, 1, None, 0, block, None, 0, None), (block, None, 1, None, 0, block, None, 0, None),
                 (block, handles, 1, None, 0, None, None, 0, None), (block, handles, 1, None, 1, block, None, 0, None), (block, handles, 0, None, 0, block, None, 0, None),
                 (block, handles, 1, None, 0, block, None, -1, None), (block, handles, 1, None, 0, block, None, 2, None)):
        assert lib.aog_install_layer_sum_cone(*args) == INVALID
        assert b"aog_install_layer_sum_cone" in lib.aog_last_error(), lib.aog_last_error()
    assert lib.aog_cone_check_geometry(None, 1, 0, 1, 16, None) == INVALID and b"aog_cone_check_geometry: null argument" in lib.aog_last_error()


def _check(geom, sizes, n_layers, N):
    lib = _lib.load()
    g = np.ascontiguousarray(geom, dtype=np.float64)
    px = (C.c_int32 * len(sizes))(*sizes)
    rc = lib.aog_cone_check_geometry(g.ctypes.data_as(C.c_void_p), n_layers, len(sizes) - n_layers, g.shape[1], N, px)
    return rc, lib.aog_last_error().decode()


def test_bad_geometry_is_refused_before_device_work():
    """The check of the installation, through the entry point that runs it without handles (no device in this process)."""
    N, sizes = 16, [16, 24, 24]      # a ground layer, a layer and a mirror on a meta-pupil of N + 8: c = 4, |s| + (1 - m) 7.5 <= 3
    good = np.zeros((3, 3, 3))
    good[:, :, 2] = 1.0
    good[1] = [(0.5, -0.25, 0.875), (2.0, -2.0, 0.875), (-1.5, 0.75, 0.8123)]
    good[2] = [(0.0, 0.0, 0.6), (3.0, -3.0, 1.0), (0.1, 0.2, 0.9)]
    assert ref.check(good, sizes, N)
    assert _check(good, sizes, 2, N)[0] == 0

    def bad(l, b, k, v, word):
        g = good.copy()
        g[l, b, k] = v
        rc, msg = _check(g, sizes, 2, N)
        assert rc == INVALID and word in msg and "aog_cone_check_geometry" in msg, (rc, msg)
        assert not ref.check(g, sizes, N)

    bad(1, 0, 2, 0.0, "magnification m = 0 of layer 1, env 0")
    bad(1, 2, 2, -0.5, "of layer 1, env 2")
    bad(2, 1, 2, 1.0000000000000002, "magnification m = 1.0000000000000002 of mirror 0, env 1")
    bad(2, 0, 2, float("nan"), "of mirror 0, env 0")
    bad(1, 1, 0, float("nan"), "shift x = nan pixels at m = 0.875 of layer 1, env 1 is outside the margin")
    bad(1, 1, 1, float("inf"), "shift y = inf")
    bad(1, 1, 0, 2.25, "shift x = 2.25 pixels at m = 0.875 of layer 1, env 1 is outside the margin (|shift| + (1 - m) (N - 1) / 2 <= 3")      # 2.25 + 0.9375
    bad(2, 0, 2, 0.59, "of mirror 0, env 0 is outside the margin")      # (1 - 0.59) 7.5 = 3.075
    bad(2, 1, 1, -3.5, "shift y = -3.5")
    bad(0, 2, 0, 0.25, "of layer 0, env 2 is outside the margin (|shift| + (1 - m) (N - 1) / 2 <= 0")      # the ground layer has no margin
    bad(0, 1, 2, 0.99, "of layer 0, env 1 is outside the margin")
    for sizes_, n_layers, word in (([16, 23, 24], 2, "layer 1 has 23 pixels"), ([16, 24, 14], 2, "mirror 0 has 14 pixels"), ([16, 24, 24], 0, "0 layers")):
        rc, msg = _check(good, sizes_, n_layers, N)
        assert rc == INVALID and word in msg, msg
    rc, msg = _check(np.ones((9, 1, 3)), [16] * 9, 9, N)
    assert rc == INVALID and "at most 8 sources" in msg


def test_the_header_states_the_arithmetic():
    text = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    for phrase in ("s0 = floor(s), r = s - s0, k = m - 1", "e = k * (i - ctr)", "q = e + r", "q0 = floor(q)", "f = q - q0", "g = 1 - f", "i + s0 + q0",
                   "never a fused multiply-add",
                   "v_l = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))", "0 < m <= 1", "|s| + (1 - m) (N - 1) / 2 <= c_l - 1",
                   "the index and the weights of aogym_sightline.h to the bit", "p - floor(p)",
                   "the bits of aog_install_layer_sum_conjugate, at whole-pixel and at fractional shifts", "ctr = (N - 1) / 2"):
        assert phrase in text, phrase


# ---- the stream-coverage rule for this header ------------------------------------------------------------------------------------------------
def _tables():
    with open(os.path.join(ROOT, "tests", "test_gpu_cone.py")) as f:
        tree = ast.parse(f.read())
    found, tests = {}, set()
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("COVERED", "NOT_DRIVEN"):
            found[node.targets[0].id] = ast.literal_eval(node.value)
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            tests.add(node.name)
    return found["COVERED"], found["NOT_DRIVEN"], tests


def _problems(text):
    names = stream_entry_points(text)
    covered, not_driven, tests = _tables()
    lines = []
    if not names or len(names) != len(set(names)):
        lines.append(f"the header parse found {len(names)} names, {len(set(names))} distinct")
    lines += [f"{n}: in COVERED and in NOT_DRIVEN" for n in set(covered) & set(not_driven)]
    lines += [f"{n}: an entry point with a stream parameter that test_gpu_cone.py places nowhere" for n in names if n not in covered and n not in not_driven]
    lines += [f"{n}: placed, but not (or no longer) declared with a stream parameter" for n in list(covered) + list(not_driven) if n not in names]
    lines += [f"{n}: COVERED names {t}, which test_gpu_cone.py does not define" for n, t in covered.items() if t not in tests]
    for n, reason in not_driven.items():
        if not (isinstance(reason, str) and reason.strip()):
            lines.append(f"{n}: NOT_DRIVEN gives no reason")
        if _python_callers(n):
            lines.append(f"{n} is in NOT_DRIVEN but {_python_callers(n)} call it: drive it on a side stream")
    return lines


def test_every_stream_entry_point_is_placed():
    assert stream_entry_points(_header()) == ["aog_install_layer_sum_cone"]      # (aog_cone_check_geometry has no stream: host only)
    lines = _problems(_header())
    assert not lines, "\n".join(lines)
    assert _problems(_header() + "\nint aog_z(aog_env*,\n          void* stream);\n") == [
        "aog_z: an entry point with a stream parameter that test_gpu_cone.py places nowhere"]
    assert "layered.py" in _python_callers("aog_install_layer_sum_cone")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def _aperture(N):
    yy, xx = np.mgrid[:N, :N]
    ctr = 0.5 * (N - 1)
    return np.flatnonzero(((yy - ctr) ** 2 + (xx - ctr) ** 2 <= (N / 2) ** 2).ravel()).astype(np.int32)


def test_a_ramp_is_seen_shrunk_by_m():
    """A layer that is a pure ramp g x is seen, after the mean is removed, as the ramp m g x: bilinear reads are exact on linear functions,
    so only rounding remains — held to 1e-12 of the peak."""
    N, n, B = 16, 24, 3
    ap = _aperture(N)
    iy, ix = np.divmod(ap, N)
    slope = 3e-7
    layer = np.tile(slope * np.arange(n, dtype=np.float64)[None, None, :], (B, n, 1))
    geom = np.array([[(0.5, -0.25, 0.875), (0.0, 0.0, 1.0), (-1.5, 0.75, 0.8123)]]).reshape(1, B, 3)
    assert ref.check(geom, [n], N)
    out = ref.install([layer], geom, ap, N, 1.5e-6)
    for b in range(B):
        want = geom[0, b, 2] * slope * (ix - ix.mean())
        assert np.abs(out["psi64"][b] - want).max() <= 1e-12 * np.abs(want).max(), b
    # and a y-ramp likewise, with its own shift
    out = ref.install([layer.transpose(0, 2, 1).copy()], geom, ap, N, 1.5e-6)
    for b in range(B):
        want = geom[0, b, 2] * slope * (iy - iy.mean())
        assert np.abs(out["psi64"][b] - want).max() <= 1e-12 * np.abs(want).max(), b


def test_host_restatement_against_the_sightline_restatement():
    rng = np.random.RandomState(3)
    N, n, B = 16, 24, 3
    ap = _aperture(N)
    ground, high = rng.randn(B, N, N) * 1e-6, rng.randn(B, n, n) * 1e-6
    # m = 1 and whole-pixel shifts: the sightline restatement's bits
    whole = np.array([[0.0, 0.0], [3.0, -2.0], [-3.0, 1.0]])
    shifts = np.stack([np.zeros((B, 2)), whole])
    geom = np.concatenate([shifts, np.ones((2, B, 1))], axis=2)
    a, b = ref.install([ground, high], geom, ap, N, 1.5e-6), sref.install([ground, high], shifts, ap, N, 1.5e-6)
    np.testing.assert_array_equal(a["psi64"], b["psi64"]), np.testing.assert_array_equal(a["tiles"], b["tiles"])
    # m = 1 and fractional shifts: the correction is an exact zero and the weights are the sightline header's, so the same bits — also for the m = 1 envs of a
    # batch that holds others (an env's bits do not depend on the batch it sits in)
    frac = np.array([[0.3, -0.7], [2.25, -1.5], [-2.9, 0.1]])
    shifts[1], geom[1, :, :2] = frac, frac
    a, b = ref.install([ground, high], geom, ap, N, 1.5e-6), sref.install([ground, high], shifts, ap, N, 1.5e-6)
    np.testing.assert_array_equal(a["psi64"].view(np.uint64), b["psi64"].view(np.uint64))
    mixed = geom.copy()
    mixed[1, 1, 2] = 0.9
    c = ref.install([ground, high], mixed, ap, N, 1.5e-6)
    np.testing.assert_array_equal(c["psi64"][[0, 2]].view(np.uint64), b["psi64"][[0, 2]].view(np.uint64))
    assert not np.array_equal(c["psi64"][1], b["psi64"][1])
    # the chain, element by element, at one pixel
    g = np.array([[(0.5, -0.25, 0.875)] * B])
    v = ref.cone_layer(high, g[0], ap, N)
    p = 37
    iy, ix = divmod(int(ap[p]), N)
    ctr, c = 7.5, 4
    k = 0.875 - 1.0
    qy, qx = (k * (iy - ctr)) + (-0.25 - -1.0), (k * (ix - ctr)) + (0.5 - 0.0)
    fy, fx = qy - np.floor(qy), qx - np.floor(qx)
    y0, x0 = iy + -1 + int(np.floor(qy)), ix + 0 + int(np.floor(qx))
    gy, gx = 1.0 - fy, 1.0 - fx
    s = high[1]
    want = (gy * ((gx * s[c + y0, c + x0]) + (fx * s[c + y0, c + x0 + 1]))) + (fy * ((gx * s[c + y0 + 1, c + x0]) + (fx * s[c + y0 + 1, c + x0 + 1])))
    assert v[1, p] == want
    # x and -x are exact negatives: a mirror that holds minus a layer at its altitude cancels it exactly, whatever the geometry
    both = np.concatenate([g, g])
    assert not ref.cone_sum([high, -high], both, ap, N).any()


def test_displaced_basis_with_a_magnification_equals_the_cone_read():
    rng = np.random.RandomState(4)
    N, M, K = 16, 24, 5
    ap = _aperture(N)
    basis = rng.randn(K, M, M)
    for sx, sy, m in ((0.5, -0.25, 0.875), (-1.5, 0.75, 0.8123), (2.0, -1.0, 1.0), (0.3, 0.3, 1.0)):
        got = tm.displaced_basis(basis, (sx, sy), ap, N, m)
        want = ref.cone_layer(basis, np.tile([sx, sy, m], (K, 1)), ap, N)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    np.testing.assert_array_equal(tm.displaced_basis(basis, (0.3, 0.3), ap, N, 1.0), tm.displaced_basis(basis, (0.3, 0.3), ap, N))
    # without a magnification it is the sightline read, as before
    np.testing.assert_array_equal(tm.displaced_basis(basis, (0.3, 0.3), ap, N), sref.displaced_layer(basis, np.tile([0.3, 0.3], (K, 1)), ap, N))
    tables = types.SimpleNamespace(ap_index=ap, modes=rng.randn(ap.size, 3))
    T = tm.sightline_shapes(tables, [basis], [(0.5, -0.25)], num_pupil_pixels=N, magnifications=[np.array([0.875, 0.875])])
    np.testing.assert_array_equal(T[3:], tm.displaced_basis(basis, (0.5, -0.25), ap, N, 0.875) / (2.0 * np.pi))
    with pytest.raises(ValueError, match="differs across the batch"):
        tm.sightline_shapes(tables, [basis], [(0.5, -0.25)], num_pupil_pixels=N, magnifications=[np.array([0.875, 0.9])])
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        tm.sightline_shapes(tables, [basis], [(0.5, -0.25)], num_pupil_pixels=N, magnifications=[1.5])


# ---- tilt_blind ------------------------------------------------------------------------------------------------------------------------------
def test_tilt_blind_projects_tip_and_tilt_out():
    rng = np.random.RandomState(6)
    N, M, K = 16, 24, 9
    ap = _aperture(N)
    iy, ix = np.divmod(ap, N)
    from adaptive_optics_gym_amd.conjugate import influence_basis

    basis = influence_basis(M, 3)
    tables = types.SimpleNamespace(ap_index=ap, modes=np.zeros((ap.size, 0)))
    T_lgs = tm.sightline_shapes(tables, [basis], [(0.5, -0.25)], pupil_mirror=False, num_pupil_pixels=N, magnifications=[0.875])
    T_ngs = tm.sightline_shapes(tables, [basis], [(-1.5, 0.75)], pupil_mirror=False, num_pupil_pixels=N)
    P = tm.tilt_projected(T_lgs, ap, N)
    tip, tilt = ix - ix.mean(), iy - iy.mean()
    for t in (tip, tilt):
        dots = np.abs(P @ t) / (np.linalg.norm(P, axis=1) * np.linalg.norm(t))
        assert dots.max() <= 1e-12, dots.max()
    assert np.abs(T_lgs @ tip).max() > 1e-3 * np.linalg.norm(T_lgs, axis=1).max() * np.linalg.norm(tip)      # (the unprojected rows do see tilt)
    # the reconstructed command: u = - H^-1 sum_g Tc_g (w_g - mean), the normal equations solved on the host
    T = [P, T_ngs]
    H_inv = tm.reconstructor(T, [1.0, 1.0], 0.0)
    c = rng.randn(K) * 1e-7
    w = [-(c @ T_lgs), -(c @ T_ngs)]      # what a mirror holding -c would leave: the atmosphere lies in the span
    solve = lambda w: -H_inv @ sum(tm.centred(Tg) @ (wg - wg.mean()) for Tg, wg in zip(T, w))
    u = solve(w)
    junk = 3e-7 * tip - 5e-7 * tilt + 1e-7
    moved = solve([w[0] + junk, w[1]])
    assert np.abs(moved - u).max() <= 1e-9 * np.abs(u).max()
    # while the same tilt on the guide that sees it moves the answer, and without the projection it moves it on the blind one too
    assert np.abs(solve([w[0], w[1] + junk]) - u).max() > 1e-3 * np.abs(u).max()
    H_plain = tm.reconstructor([T_lgs, T_ngs], [1.0, 1.0], 0.0)
    plain = lambda w: -H_plain @ sum(tm.centred(Tg) @ (wg - wg.mean()) for Tg, wg in zip([T_lgs, T_ngs], w))
    assert np.abs(plain([w[0] + junk, w[1]]) - plain(w)).max() > 1e-3 * np.abs(u).max()
    np.testing.assert_allclose(plain(w), c, rtol=0, atol=1e-9 * np.abs(c).max())
