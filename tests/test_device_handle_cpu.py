"""The base of the stand-alone handles' wrappers (adaptive_optics_gym_amd/device_handle.py) on CPU tensors, against a stub library that
records its calls."""
import ctypes as C

import pytest
import torch

from adaptive_optics_gym_amd.device_handle import DeviceHandle, check_measurement

BYTES = 48


class _StubLib:
    """Every ``aog_stub_*`` entry point succeeds and is recorded by name; the handle it makes is 7."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            if name.endswith("_create"):
                C.cast(args[2], C.POINTER(C.c_void_p))[0] = 7
            return BYTES if name.endswith("_state_bytes") else 0

        return entry


class _Config(C.Structure):
    _fields_ = [("batch", C.c_int32)]


class _Wrapper(DeviceHandle):
    prefix, noun = "aog_stub", "stub"

    def __init__(self, batch, lazy):
        self.lazy = lazy
        self.stub = _StubLib()
        self._bind(torch, "cpu", batch)
        if not lazy:
            self._create()

    def _load(self):
        return self.stub

    def _config(self):
        return _Config(self._batch)

    def _stream(self):
        return None


def test_mask_accepts_bool_and_uint8_vectors_of_batch_entries():
    w = _Wrapper(3, lazy=False)
    assert w._mask(None, "reset") is None
    for mask in ([True, False, True], torch.tensor([1, 0, 1], dtype=torch.uint8), torch.tensor([True, False, True])):
        m = w._mask(mask, "reset")
        assert m.dtype == torch.uint8 and m.is_contiguous() and m.tolist() == [1, 0, 1]
    for bad in ([True, False], torch.ones(4, dtype=torch.bool), torch.ones(3, dtype=torch.float32), torch.ones(3, dtype=torch.int64),
                torch.ones((3, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"^update: mask must be a bool vector of 3 entries$"):
            w._mask(bad, "update")


def test_tensor_check_raises_the_callers_message():
    w = _Wrapper(3, lazy=False)
    good = torch.zeros((3, 2), dtype=torch.float64)
    assert w._tensor(good, (3, 2), torch.float64, "no") is good
    for bad in (good.float(), torch.zeros((2, 3), dtype=torch.float64), torch.zeros((3, 4), dtype=torch.float64)[:, ::2], [[0.0, 0.0]] * 3):
        with pytest.raises(ValueError, match="^who: y is wrong$"):
            w._tensor(bad, (3, 2), torch.float64, "who: y is wrong")


def test_set_state_refuses_a_wrong_blob_before_the_library_sees_it():
    w = _Wrapper(3, lazy=False)
    for bad in (torch.zeros(BYTES - 1, dtype=torch.uint8), torch.zeros(BYTES + 8, dtype=torch.uint8), torch.zeros(BYTES, dtype=torch.int8),
                torch.zeros((BYTES, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError, match=f"^set_state: the blob of this stub is a uint8 vector of {BYTES} bytes$"):
            w.set_state(bad)
    assert "aog_stub_set_state" not in w.stub.calls and w.stub.calls.count("aog_stub_create") == 1


def test_close_twice_destroys_once():
    w = _Wrapper(3, lazy=False)
    assert w.stub.calls == ["aog_stub_create"] and w._handle.value == 7
    w.close()
    w.close()
    w.__del__()
    assert w.stub.calls.count("aog_stub_destroy") == 1 and w._handle is None
    never = _Wrapper(3, lazy=True)
    never.close()
    assert never.stub.calls == [] and never.lib is None   # (no handle was ever made: nothing to destroy, the library not even loaded)


def test_a_lazy_handle_is_created_once_on_first_use():
    w = _Wrapper(3, lazy=True)
    assert w._handle is None and w.stub.calls == []
    w._mask([True, False, True], "reset")   # (argument checks need no handle)
    assert w._handle is None
    w._call("reset", None, w._stream())
    w._call("reset", None, w._stream())
    assert w._state_bytes() == BYTES
    assert w.stub.calls == ["aog_stub_create", "aog_stub_reset", "aog_stub_reset", "aog_stub_state_bytes"]
    w.close()
    assert w.stub.calls[-1] == "aog_stub_destroy"


def test_measurement_is_checked_against_the_env():
    env = type("E", (), {"pyramid": None})()
    check_measurement(env, "truth")
    with pytest.raises(ValueError, match=r"^measurement must be 'truth' or 'pyramid' \(got 'shack'\)$"):
        check_measurement(env, "shack")
    with pytest.raises(ValueError, match=r"^measurement='pyramid' needs an env created with pyramid=dict\(\.\.\.\)$"):
        check_measurement(env, "pyramid")
    check_measurement(type("E", (), {"pyramid": {"modulation": 3}})(), "pyramid")
