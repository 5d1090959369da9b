"""Altitude-conjugated mirrors, host side (no GPU): the C-ABI surface of include/aogym_conjugate.h (every refusal comes before any device
work — that this file passes without a GPU is the demonstration), the build's unit and header, the Python-side refusals that run before
anything is created, the default basis and its fit, the self-consistency of the host restatement (tests/conjugate_reference.py) and the
stream-coverage rule for the new header against the tables of tests/test_gpu_conjugate.py."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import conjugate_reference as ref
import sightline_reference as sref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd import conjugate as cj
from test_stream_coverage_cpu import ROOT, _python_callers, stream_entry_points

INVALID = -1
HANDLE_SYMBOLS = ("aog_altmirror_config_size", "aog_altmirror_create", "aog_altmirror_destroy", "aog_altmirror_upload", "aog_altmirror_set_command",
                  "aog_altmirror_get", "aog_altmirror_fit", "aog_altmirror_state_bytes", "aog_altmirror_get_state", "aog_altmirror_set_state")
NEW_SYMBOLS = HANDLE_SYMBOLS + ("aog_install_layer_sum_conjugate",)
GOOD = dict(abi_version=22, num_envs=4, n_pixels=44, n_modes=9, reserved=0)
# entry point -> the positions of the pointers it requires (masks, the stream and the optional arrays are nullable)
REQUIRED = {"aog_altmirror_upload": (0, 1), "aog_altmirror_set_command": (0, 1), "aog_altmirror_get": (0,), "aog_altmirror_fit": (0, 1, 2),
            "aog_altmirror_get_state": (0, 1), "aog_altmirror_set_state": (0, 1)}


def _header():
    with open(os.path.join(ROOT, "include", "aogym_conjugate.h")) as f:
        return f.read()


def _parameter_names(name):
    params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)).group(1).split(",")
    return [re.findall(r"\w+", p)[-1] for p in params]


# ---- the header and the handle's life ---------------------------------------------------------------------------------------------------------
def test_cabi_surface_of_the_new_header(repo_root):
    header = _header()
    lib = _lib.load()
    assert '#include "aogym.h"' in header
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(NEW_SYMBOLS) == set(_lib.CONJUGATE_SYMBOLS)
    for other in ("aogym.h", "aogym_disturbance.h", "aogym_sightline.h", "aogym_servo.h"):
        text = open(os.path.join(repo_root, "include", other)).read()
        for name in NEW_SYMBOLS:
            assert not re.search(r"\b%s\s*\(" % name, text), (other, name)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert not any(name in table for table in (_lib.SYMBOLS, _lib.DISTURBANCE_SYMBOLS, _lib.SIGHTLINE_SYMBOLS, _lib.SERVO_SYMBOLS)), name
    # a table of its own: no entry of STANDALONE, and a prefix none of the six begins
    assert "aog_altmirror" not in _lib.STANDALONE and not any("aog_altmirror".startswith(p) for p in _lib.STANDALONE)
    assert lib.aog_abi_version() == _lib.ABI_VERSION == 22
    assert lib.aog_altmirror_config_size() == C.sizeof(_lib.AogAltMirrorConfig) == 20
    assert cj.MAX_MODES == 256 and "AOG_ALTMIRROR_MAX_MODES = 256" in header


def test_destroy_and_state_bytes_of_null():
    lib = _lib.load()
    assert lib.aog_altmirror_destroy(None) is None
    assert lib.aog_altmirror_state_bytes(None) == 0


def test_create_names_its_null_argument():
    lib = _lib.load()
    cfg, out = _lib.AogAltMirrorConfig(**GOOD), C.c_void_p(0x5A5A)
    assert lib.aog_altmirror_create(None, 0, C.byref(out)) == INVALID and lib.aog_last_error().decode().endswith("aog_altmirror_create: null argument cfg")
    assert out.value == 0x5A5A
    assert lib.aog_altmirror_create(C.byref(cfg), 0, None) == INVALID and lib.aog_last_error().decode().endswith("aog_altmirror_create: null argument out")


@pytest.mark.parametrize("change,field", [(dict(abi_version=21), "abi_version"), (dict(num_envs=0), "num_envs"), (dict(num_envs=-2), "num_envs"),
                                          (dict(n_pixels=0), "n_pixels"), (dict(n_modes=0), "n_modes"), (dict(n_modes=257), "n_modes"),
                                          (dict(reserved=1), "reserved"), (dict(num_envs=2 ** 20, n_pixels=2 ** 6), "num_envs")],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_create_refuses_a_bad_config_naming_the_field(change, field):
    lib = _lib.load()
    cfg, out = _lib.AogAltMirrorConfig(**{**GOOD, **change}), C.c_void_p(0x5A5A)
    assert lib.aog_altmirror_create(C.byref(cfg), 0, C.byref(out)) == INVALID
    message = lib.aog_last_error().decode()
    assert "aog_altmirror_create" in message and field in message, message
    assert not out.value


@pytest.mark.parametrize("name,position", [(n, p) for n, ps in REQUIRED.items() for p in ps])
def test_a_null_argument_is_named_before_anything_is_dereferenced(name, position):
    """The handle the calls get is a block of zeros: a refusal that looked at it first would not name the argument."""
    lib = _lib.load()
    keep = [C.create_string_buffer(4096) for _ in _lib.CONJUGATE_SYMBOLS[name][1]]
    args = [C.c_void_p(C.addressof(k)) for k in keep]
    args[position] = None
    assert getattr(lib, name)(*args) == INVALID
    assert lib.aog_last_error().decode().endswith(f"{name}: null argument {_parameter_names(name)[position]}")
    # several nulls name the first in the parameter list
    for p in REQUIRED[name]:
        args[p] = None
    assert getattr(lib, name)(*args) == INVALID
    assert lib.aog_last_error().decode().endswith(f"{name}: null argument {_parameter_names(name)[REQUIRED[name][0]]}")


def test_the_installation_refuses_null_arguments():
    lib = _lib.load()
    assert lib.aog_install_layer_sum_conjugate(None, None, 1, None, 0, None, None, 0, None) == INVALID
    assert b"aog_install_layer_sum_conjugate" in lib.aog_last_error()


def test_the_build_holds_the_unit_and_the_header():
    build = __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"])
    assert "conjugate" in build.UNITS and set(build.EXTRA_HEADERS["aogym_conjugate.h"]) == {"layers", "conjugate"}
    assert any(p.endswith("aogym_conjugate.h") for p in build.source_files())
    for unit in ("conjugate", "layers"):
        deps = build._unit_deps(unit)
        assert any(p.endswith("aogym_conjugate.h") for p in deps) and any(p.endswith("conjugate_host.h") for p in deps), unit
    assert any(p.endswith("k_conjugate.h") for p in build._unit_deps("conjugate"))


def test_the_header_states_the_arithmetic():
    text = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    for phrase in ("s = cmd[b][0] basis[0][p]", "never a fused multiply-add", "never a matrix instruction", "M M 2^-53 sum_p |fit[k][p] screen_b[p]|",
                   "n_layers + n_mirrors <= 8", "ring origin 0", "2 pi x metres of optical path"):
        assert phrase in text, phrase


# ---- the stream-coverage rule for this header ------------------------------------------------------------------------------------------------
def _tables():
    with open(os.path.join(ROOT, "tests", "test_gpu_conjugate.py")) as f:
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
    lines += [f"{n}: an entry point with a stream parameter that test_gpu_conjugate.py places nowhere" for n in names
              if n not in covered and n not in not_driven]
    lines += [f"{n}: placed, but not (or no longer) declared with a stream parameter" for n in list(covered) + list(not_driven) if n not in names]
    lines += [f"{n}: COVERED names {t}, which test_gpu_conjugate.py does not define" for n, t in covered.items() if t not in tests]
    for n, reason in not_driven.items():
        if not (isinstance(reason, str) and reason.strip()):
            lines.append(f"{n}: NOT_DRIVEN gives no reason")
        if _python_callers(n):
            lines.append(f"{n} is in NOT_DRIVEN but {_python_callers(n)} call it: drive it on a side stream")
    return lines


def test_the_header_declares_the_stream_entry_points():
    assert stream_entry_points(_header()) == ["aog_altmirror_upload", "aog_altmirror_set_command", "aog_altmirror_get", "aog_altmirror_fit",
                                              "aog_altmirror_get_state", "aog_altmirror_set_state", "aog_install_layer_sum_conjugate"]


def test_every_stream_entry_point_is_placed():
    lines = _problems(_header())
    assert not lines, "\n".join(lines)


def test_a_new_stream_entry_point_is_reported():
    lines = _problems(_header() + "\nint aog_z(aog_altmirror*,\n          void* stream);\n")
    assert lines == ["aog_z: an entry point with a stream parameter that test_gpu_conjugate.py places nowhere"]


def test_the_python_callers_are_found():
    for name in stream_entry_points(_header()):
        assert "conjugate.py" in _python_callers(name), name


# ---- Python-side refusals, before anything is created ---------------------------------------------------------------------------------------
LAYERS = [{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}]
EIGHT = [{"fraction": 0.125, "speed": 30.0}] * 8
MIRROR = dict(altitude=1e4, actuators=3)


@pytest.mark.parametrize("kw,word", [
    (dict(altitude_mirrors=[MIRROR]), "altitude_mirrors need layer_altitudes"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_action=1e-7), "altitude_action needs altitude_mirrors"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[MIRROR] * 7), "2 layers and 7 altitude mirrors"),
    (dict(atm_layers=EIGHT, layer_altitudes=[0.0] * 8, altitude_mirrors=[MIRROR]), "at most 8 sources"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(actuators=3)]), "every mirror is a dict with 'altitude'"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=-1.0)]), ">= 0"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=1e4, stroke=1.0)]), "every mirror is a dict"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=1e4, actuators=17)]), "actuators"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=1e4, coupling=1.0)]), "coupling"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=1e4, basis=np.zeros((4, 40, 40)))], meta_pupil_pixels=44), r"\[K, 44, 44\]"),
    (dict(layer_altitudes=[0.0, 1e4], altitude_mirrors=[MIRROR], altitude_action=float("nan")), "finite scale"),
    # a sightline inside the layers' margin but outside a higher mirror's: 3.2 pixels at 10 km pass c = 6, 6.4 pixels at 20 km do not
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=44, altitude_mirrors=[dict(altitude=2e4)], sightlines={"uplink": (5e-6, 0.0)}),
     "sightline 'uplink': mirror 0 .* leaves 5"),
    (dict(layer_altitudes=[0.0, 1e4], meta_pupil_pixels=44, altitude_mirrors=[MIRROR, dict(altitude=2e4)], field_angle=(0.0, -5e-6)),
     "field_angle: mirror 1 .* leaves 5"),
])
def test_mirrors_are_refused_before_anything_is_created(kw, word, monkeypatch):
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    def never(self, *a, **k):
        raise AssertionError("the env was being created")

    monkeypatch.setattr(BatchedAOEnv, "__init__", never)
    args = dict(atm_layers=LAYERS, atm_fried=0.15, act_type="zernike", act_dim=6, num_pupil_pixels=32, verbose=False)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        LayeredAOEnv(2, "cuda:0", **args)


def test_the_mirrors_altitudes_count_in_the_default_margin():
    """Without the mirror 3.2 pixels ask for c = 5 (N_L = 44); a mirror at 20 km is read 6.4 pixels off: c = 8, N_L = 48."""
    from adaptive_optics_gym_amd import layered as L

    angle = L.resolve_field_angle((5e-6, 0.0), 2)
    pitch = 0.5 / 32
    assert L.default_meta_pupil_pixels(32, L.required_margin(np.array([0.0, 1e4]), [angle], pitch)) == 44
    assert L.default_meta_pupil_pixels(32, L.required_margin(np.array([0.0, 1e4, 2e4]), [angle], pitch)) == 48
    with pytest.raises(ValueError, match="angle: layer 1 "):
        L.check_margin(L.sightline_shifts(np.array([0.0, 2e4]), angle, pitch), [0, 6], "angle")
    with pytest.raises(ValueError, match="angle: mirror 0 "):
        L.check_margin(L.sightline_shifts(np.array([0.0, 2e4]), angle, pitch), [0, 6], "angle", first_mirror=1)


# ---- the default basis and the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(44, 9), (32, 9), (44, 3), (7, 1)])
def test_default_basis_and_its_fit(M, n):
    basis = cj.influence_basis(M, n, 0.15)
    K = n * n
    assert basis.shape == (K, M, M) and basis.dtype == np.float64 and basis.flags.c_contiguous
    # the peak is 2 pi at the actuator (the corner actuators sit on the corner pixels) and `coupling` of it one pitch away
    peak = basis[0, 0, 0] if n > 1 else basis[0, M // 2, M // 2]      # (one actuator alone sits at the centre)
    assert abs(peak - 2 * np.pi) < 1e-12 and abs(basis.max() - 2 * np.pi) < 1e-12
    if n > 1:
        centres = np.linspace(0, M - 1, n)
        g = lambda x, c: np.exp(np.log(0.15) * ((x - c) / (centres[1] - centres[0])) ** 2)
        assert abs(g(centres[1], centres[0]) - 0.15) < 1e-15
        j, i = 1, n - 1
        yy, xx = np.mgrid[:M, :M]
        np.testing.assert_allclose(basis[j * n + i], 2 * np.pi * g(yy, centres[j]) * g(xx, centres[i]), rtol=0, atol=1e-12)
    fit = cj.fit_matrix(basis)
    assert fit.shape == (K, M * M) and fit.flags.c_contiguous
    c = np.random.RandomState(M + n).randn(K, 5)
    np.testing.assert_allclose(fit @ (basis.reshape(K, -1).T @ c), c, rtol=0, atol=1e-10)      # pinv(basis) basis c = c
    np.testing.assert_allclose(np.linalg.pinv(basis.reshape(K, -1).T) @ basis.reshape(K, -1).T @ c, c, rtol=0, atol=1e-10)


def test_host_restatement_of_surface_fit_and_installation():
    rng = np.random.RandomState(5)
    B, K, M, N = 3, 4, 12, 8
    basis, cmd = rng.randn(K, M, M), rng.randn(B, K) * 1e-7
    s = ref.surface(cmd, basis)
    # the header's chain, element by element, and its order (a reversed sum differs in the last bits somewhere)
    for b, p in ((0, 0), (1, 77), (2, M * M - 1)):
        v = cmd[b, 0] * basis[0].ravel()[p]
        for k in range(1, K):
            v = v + (cmd[b, k] * basis[k].ravel()[p])
        assert s[b, p] == v
    assert not np.array_equal(s, ref.surface(cmd[:, ::-1], basis[::-1]))
    np.testing.assert_allclose(s, cmd @ basis.reshape(K, -1), rtol=0, atol=1e-20)
    np.testing.assert_array_equal(ref.surface(cmd[:, :1], basis[:1]), cmd[:, :1] * basis[0].ravel()[None, :])      # K = 1: one product
    np.testing.assert_array_equal(ref.surface(-cmd, basis), -s)       # x and -x are exact negatives
    # a masked set_command keeps the other envs' command and surface
    c0, s0 = rng.randn(B, K), rng.randn(B, M * M)
    c1, s1 = ref.set_command(c0, s0, cmd, basis, mask=[1, 0, 1])
    np.testing.assert_array_equal(c1[1], c0[1]), np.testing.assert_array_equal(s1[1], s0[1])
    np.testing.assert_array_equal(c1[[0, 2]], cmd[[0, 2]]), np.testing.assert_array_equal(s1[[0, 2]], s[[0, 2]])
    # the fit gives a command back within its own bound
    fit = cj.fit_matrix(basis)
    value, bound = ref.fit(fit, s.reshape(B, M, M))
    assert np.all(np.abs(value - cmd) <= 4 * bound) and bound.min() > 0
    # the installation: the mirror is one more source, added with a plus sign; minus the layer's own screen cancels it exactly
    ap = np.arange(N * N)
    layer = rng.randn(B, M, M) * 1e-6
    shifts = np.stack([np.tile([0.25, -1.5], (B, 1))] * 2)
    out = ref.install([layer], [-layer], shifts, ap, N, 1.5e-6)
    assert not out["psi64"].any() and not out["s"].any()
    both = ref.install([layer], [layer], shifts, ap, N, 1.5e-6)
    np.testing.assert_array_equal(both["s"], 2 * sref.sightline_sum([layer], shifts[:1], ap, N))
    np.testing.assert_array_equal(ref.install([layer], [], shifts[:1], ap, N, 1.5e-6)["psi64"], sref.install([layer], shifts[:1], ap, N, 1.5e-6)["psi64"])
