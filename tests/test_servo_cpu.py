"""Mirror servo, host side (no GPU): the self-consistency of the host restatement (tests/servo_reference.py) the GPU tests compare with,
the argument checks of ``servo.py`` and the C-ABI surface of include/aogym_servo.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import servo_reference as ref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.servo import MAX_ACT, MAX_LATENCY, resolve_servo, resolve_stuck

NEW_SYMBOLS = ("aog_servo_config_size", "aog_servo_create", "aog_servo_destroy", "aog_servo_set_params", "aog_servo_reset", "aog_servo_apply",
               "aog_servo_state_bytes", "aog_servo_get_state", "aog_servo_set_state")


def _actions(rng, T, B, A):
    return rng.randn(T, B, A).astype(np.float32)


@pytest.mark.parametrize("d", [0, 1, 2, 4])
def test_an_integer_latency_is_a_pure_shift(d):
    rng = np.random.RandomState(d)
    a = _actions(rng, 9, 3, 5)
    s = ref.Servo(3, 5, 4, latency=float(d))
    out = np.stack([s.apply(x) for x in a])
    np.testing.assert_array_equal(out[:d].view(np.uint32), np.zeros((d, 3, 5), dtype=np.uint32))   # the rest command, before the first frame
    np.testing.assert_array_equal(out[d:].view(np.uint32), a[:9 - d].view(np.uint32))


def test_a_fractional_latency_interpolates_and_the_identity_keeps_the_bits():
    rng = np.random.RandomState(1)
    a = _actions(rng, 6, 2, 4)
    a[0, 0, 0] = -0.0
    s = ref.Servo(2, 4, 2, latency=np.array([1.5, 0.0]))
    out = np.stack([s.apply(x) for x in a])
    np.testing.assert_array_equal(out[:, 1].view(np.uint32), a[:, 1].view(np.uint32))
    for t in range(2, 6):
        want = (0.5 * a[t - 1, 0].astype(np.float64) + 0.5 * a[t - 2, 0].astype(np.float64)).astype(np.float32)
        np.testing.assert_array_equal(out[t, 0], want)
    np.testing.assert_array_equal(out[0, 0], 0 * a[0, 0])
    np.testing.assert_array_equal(out[1, 0], (0.5 * a[0, 0].astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("alpha", [0.5, 0.1])
def test_step_response_of_the_first_order_filter(alpha):
    """A unit step through response = alpha reads 1 - (1 - alpha)^k after k frames, to rounding; response = 1 is the identity on c."""
    s = ref.Servo(1, 1, 0, response=alpha)
    one = np.ones((1, 1), dtype=np.float32)
    for k in range(1, 40):
        s.apply(one)
        want = 1.0 - (1.0 - alpha) ** k
        assert abs(s.y[0, 0] - want) <= 4 * k * 2.0 ** -53
    rng = np.random.RandomState(2)
    a = _actions(rng, 5, 2, 3)
    s = ref.Servo(2, 3, 1, latency=1.0, response=1.0, stroke=0.5)
    out = np.stack([s.apply(x) for x in a])
    np.testing.assert_array_equal(out[1:], np.clip(a[:-1], -0.5, 0.5))
    assert np.abs(a).max() > 0.5   # (the clip had something to do)


def test_stroke_stuck_mask_and_reset():
    rng = np.random.RandomState(3)
    B, A = 3, 4
    stuck = np.zeros((B, A), dtype=bool)
    stuck[:, 1] = True
    stuck[2, 3] = True
    val = np.where(stuck, np.float32(0.25), np.float32(0)).astype(np.float32)
    s = ref.Servo(B, A, 1, latency=1.0, stroke=np.array([np.inf, 0.3, 0.3]), stuck=stuck, stuck_value=val)
    a = _actions(rng, 6, B, A) * 2
    out0 = s.apply(a[0])
    assert np.all(out0[stuck] == np.float32(0.25)) and not out0[~stuck].any()
    out1 = s.apply(a[1])
    np.testing.assert_array_equal(out1[0, ~stuck[0]], a[0, 0, ~stuck[0]])                       # no stroke limit on env 0
    np.testing.assert_array_equal(out1[1, ~stuck[1]], np.clip(a[0, 1], -0.3, 0.3).astype(np.float32)[~stuck[1]])
    assert np.all(out1[stuck] == np.float32(0.25)) and np.abs(s.y[1:]).max() <= 0.3           # the filter state is the clipped drive
    # a masked call: env 1 keeps ring and y, its row of the output is not written, the counter moves for everyone
    mask = np.array([True, False, True])
    y1, ring1 = s.y[1].copy(), s.ring[1].copy()
    sentinel = np.full((B, A), np.float32(7))
    out2 = s.apply(a[2], mask, out=sentinel)
    assert np.all(out2[1] == 7) and np.array_equal(s.y[1], y1) and np.array_equal(s.ring[1], ring1) and s.n == 3
    # env 1 reads at its next call what its slot held: with R = 3 and latency 1 that is slot (3 - 1) % 3 = 2, never written: 0
    out3 = s.apply(a[3])
    assert not out3[1, ~stuck[1]].any()
    np.testing.assert_array_equal(out3[0, ~stuck[0]], a[2, 0, ~stuck[0]])
    # a masked reset restarts those envs' history alone
    s.reset(np.array([True, False, False]))
    out4 = s.apply(a[4])
    assert not out4[0, ~stuck[0]].any() and not s.y[0].any()
    np.testing.assert_array_equal(out4[2, ~stuck[2]], np.clip(a[3, 2], -0.3, 0.3)[~stuck[2]])
    assert s.blob().size == 8 * B * A + 8 + 4 * B * 3 * A


def test_parts_of_a_batch_reproduce_the_whole():
    rng = np.random.RandomState(4)
    lat, resp = np.array([0.0, 1.5, 2.0]), np.array([1.0, 0.5, 0.1])
    whole = ref.Servo(3, 5, 2, latency=lat, response=resp)
    parts = [ref.Servo(2, 5, 2, latency=lat[:2], response=resp[:2]), ref.Servo(1, 5, 2, latency=lat[2:], response=resp[2:])]
    for x in _actions(rng, 8, 3, 5):
        np.testing.assert_array_equal(whole.apply(x), np.concatenate([parts[0].apply(x[:2]), parts[1].apply(x[2:])]))


def test_argument_validation_raises_before_creation():
    ok = resolve_servo(3, 3, 0, 5, latency=[0.0, 1.5, 2.0], response=0.5, stroke=[1.0, np.inf, 2.0], stuck={1: 0.25})
    assert ok["max_latency"] == 2 and ok["stroke"][1] == np.inf and ok["stuck"][:, 1].all() and ok["stuck"].sum() == 3
    assert ok["stuck"].dtype == np.uint8 and ok["stuck_value"].dtype == np.float32 and ok["latency"].dtype == np.float64
    assert resolve_servo(2, 2, 0, 4)["max_latency"] == 0 and np.all(resolve_servo(2, 2, 0, 4)["stroke"] == np.inf)
    # total_envs values are indexed by the global env id
    cut = resolve_servo(2, 4, 2, 3, latency=[0.0, 1.0, 2.0, 3.0], stroke=[1.0, 2.0, np.inf, 4.0])
    np.testing.assert_array_equal(cut["latency"], [2.0, 3.0])
    np.testing.assert_array_equal(cut["stroke"], [np.inf, 4.0])
    assert cut["max_latency"] == 3
    bad = [dict(latency=-0.5), dict(latency=4.5), dict(latency=2.0, max_latency=1), dict(max_latency=5), dict(max_latency=-1), dict(max_latency=1.5),
           dict(latency=float("nan")), dict(latency=[0.0, 1.0]), dict(response=0.0), dict(response=1.5), dict(response=-0.1), dict(stroke=0.0),
           dict(stroke=-1.0), dict(stroke=float("nan")), dict(stroke=-np.inf), dict(stuck={5: 0.0}), dict(stuck={-1: 0.0}), dict(stuck={0: float("inf")}),
           dict(stuck={0.5: 0.0}), dict(stuck=[1, 2, 3]), dict(stuck=(np.zeros(4, dtype=bool), np.zeros(5))),
           dict(stuck=(np.ones(5, dtype=bool), np.full(5, np.nan)))]
    for kw in bad:
        with pytest.raises(ValueError):
            resolve_servo(3, 3, 0, 5, **kw)
    for act_dim in (0, MAX_ACT + 1):
        with pytest.raises(ValueError, match="act_dim"):
            resolve_servo(3, 3, 0, act_dim)
    m, v = resolve_stuck((np.array([True, False, True]), np.array([0.5, np.nan, -0.5])), 2, 3)   # (a value under no mask is not read)
    assert m.tolist() == [[1, 0, 1]] * 2 and v.tolist() == [[0.5, 0.0, -0.5]] * 2
    assert (MAX_LATENCY, MAX_ACT) == (4, 128)


def test_cabi_surface_of_the_new_header(repo_root):
    """Declared in include/aogym_servo.h, bound, exported; null arguments return AOG_ERR_INVALID naming the entry point; the ABI version and
    the other headers' symbol sets are untouched."""
    header = open(os.path.join(repo_root, "include", "aogym_servo.h")).read()
    lib = _lib.load()
    assert '#include "aogym.h"' in header
    declared = set(re.findall(r"\b(aog_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(NEW_SYMBOLS) == set(_lib.SERVO_SYMBOLS)
    for other in ("aogym.h", "aogym_disturbance.h", "aogym_sightline.h"):
        text = open(os.path.join(repo_root, "include", other)).read()
        for name in NEW_SYMBOLS:
            assert not re.search(r"\b%s\s*\(" % name, text), (other, name)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name not in _lib.SYMBOLS and name not in _lib.DISTURBANCE_SYMBOLS and name not in _lib.SIGHTLINE_SYMBOLS, name
    assert lib.aog_abi_version() == _lib.ABI_VERSION == 22
    assert lib.aog_servo_config_size() == ctypes.sizeof(_lib.AogServoConfig) == 16
    null = None
    calls = {"aog_servo_create": (null, 0, null), "aog_servo_set_params": (null,) * 6, "aog_servo_reset": (null,) * 3, "aog_servo_apply": (null,) * 5,
             "aog_servo_get_state": (null,) * 3, "aog_servo_set_state": (null,) * 3}
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1 and name.encode() in lib.aog_last_error(), name
    # ... and the argument: the first null pointer by the header's name (a non-null handle is never dereferenced before the check)
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    named = {"aog_servo_create": [((null, 0, ctypes.byref(ctypes.c_void_p())), b"cfg"), ((ctypes.byref(_lib.AogServoConfig(22, 4, 2, 1)), 0, null), b"out")],
             "aog_servo_set_params": [((null,) + (some,) * 5, b"servo"), ((some, null, some, some, some, some), b"latency_host"),
                                      ((some, some, null, some, some, some), b"response_host"), ((some, some, some, null, some, some), b"stroke_host"),
                                      ((some, some, some, some, null, some), b"stuck_host"), ((some,) * 5 + (null,), b"stuck_value_host")],
             "aog_servo_reset": [((null, some, some), b"servo")],
             "aog_servo_apply": [((null, some, null, some, null), b"servo"), ((some, null, null, some, null), b"action_in_dev"),
                                 ((some, some, null, null, null), b"action_out_dev")],
             "aog_servo_get_state": [((null, some, null), b"servo"), ((some, null, null), b"blob_dev")],
             "aog_servo_set_state": [((null, some, null), b"servo"), ((some, null, null), b"blob_dev")]}
    for name, cases in named.items():
        for args, word in cases:
            assert getattr(lib, name)(*args) == -1 and lib.aog_last_error().endswith(name.encode() + b": null argument " + word), (name, word)
    assert lib.aog_servo_state_bytes(None) == 0
    lib.aog_servo_destroy(None)
    # the config's own checks need no device either
    out = ctypes.c_void_p()
    for cfg, word in ((_lib.AogServoConfig(21, 4, 2, 1), b"abi_version"), (_lib.AogServoConfig(22, 0, 2, 1), b"num_envs"),
                      (_lib.AogServoConfig(22, 4, 0, 1), b"act_dim"), (_lib.AogServoConfig(22, 4, 129, 1), b"act_dim"),
                      (_lib.AogServoConfig(22, 4, 2, -1), b"max_latency"), (_lib.AogServoConfig(22, 4, 2, 5), b"max_latency"),
                      (_lib.AogServoConfig(22, 2 ** 30, 128, 4), b"num_envs")):
        assert lib.aog_servo_create(ctypes.byref(cfg), 0, ctypes.byref(out)) == -1 and b"aog_servo_create" in lib.aog_last_error()
        assert word in lib.aog_last_error() and not out.value
    build = __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"])
    assert "servo" in build.UNITS and any(p.endswith("aogym_servo.h") for p in build.source_files())
    assert any(p.endswith("aogym_servo.h") for p in build._unit_deps("servo")) and any(p.endswith("k_servo.h") for p in build._unit_deps("servo"))
