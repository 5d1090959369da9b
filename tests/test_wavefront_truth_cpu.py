"""Residual wavefront statistics and the best-fit mirror command, the parts that need no GPU: the host identities of the definition in
include/aogym.h (``optics_host.wavefront_fit`` and the route through P against tests/wavefront_reference.py's least squares), the C ABI, and
the clean failure of both entry points without a handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import wavefront_reference as wr
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.optics_host import build_tables
from adaptive_optics_gym_amd.params import OpticalParams

N = 32
BOUND = 1e-10
_TABLES = {}


def _tables(act_type, A):
    if (act_type, A) not in _TABLES:
        _TABLES[act_type, A] = build_tables(OpticalParams(num_pupil_pixels=N), act_type, A, 2)
    return _TABLES[act_type, A]


def _p_route(w, modes, act, P):
    """The definition, through P as the library takes it."""
    n = w.shape[1]
    Mc = modes - modes.mean(axis=0)
    rms = w.std(axis=1)
    b = w @ Mc
    c = b @ P.T
    fit = np.sqrt(np.maximum(0.0, rms ** 2 - np.einsum("ek,ek->e", b, c) / n))
    return dict(rms=rms, fit_rms=fit, coef=c, ideal_actuators=act - c / 2.0)


@pytest.mark.parametrize("act_type,A", [("zernike", 6), ("num_actuators", 20)], ids=["zernike6_rank_deficient", "disk20"])
def test_host_identities(act_type, A):
    from adaptive_optics_gym_amd.optics_host import wavefront_fit
    from helpers import smooth_screens

    t = _tables(act_type, A)
    assert t.n_ap == 812   # 26 pixel tiles, 12 pixels in the last
    B = 5
    rng = np.random.RandomState(3)
    act = rng.randn(B, A) * 5e-8
    w = wr.path_error(smooth_screens(B, N, 11), act, t)
    P = wavefront_fit(t.modes)
    assert P.shape == (A, A) and np.allclose(P, P.T, rtol=0, atol=1e-12 * np.abs(P).max())
    got, ref = _p_route(w, t.modes, act, P), wr.truth_of(w, t.modes, act)
    for e in range(B):
        cmax = np.abs(ref["coef"][e]).max()
        print(f"{act_type}-{A} env {e}: rms {ref['rms'][e]:.4e} fit_rms {ref['fit_rms'][e]:.4e} "
              f"d fit {abs(got['fit_rms'][e] - ref['fit_rms'][e]) / ref['rms'][e]:.2e} d coef {np.abs(got['coef'][e] - ref['coef'][e]).max() / cmax:.2e}")
        assert abs(got["rms"][e] - ref["rms"][e]) <= BOUND * ref["rms"][e]
        assert abs(got["fit_rms"][e] - ref["fit_rms"][e]) <= BOUND * ref["rms"][e]
        assert np.abs(got["coef"][e] - ref["coef"][e]).max() <= BOUND * cmax
        assert np.abs(got["ideal_actuators"][e] - ref["ideal_actuators"][e]).max() <= BOUND * np.abs(ref["ideal_actuators"][e]).max()
    if act_type == "zernike":   # Zernike 1 is piston: coefficient 0, actuator unchanged
        assert np.abs(got["coef"][:, 0]).max() <= BOUND * np.abs(got["coef"]).max()
        assert np.abs(got["ideal_actuators"][:, 0] - act[:, 0]).max() <= BOUND * np.abs(act).max()
    # closing the loop on the host: the ideal actuators leave exactly the fitting error, and nothing more to fit
    w2 = wr.path_error(smooth_screens(B, N, 11), got["ideal_actuators"], t)
    again = _p_route(w2, t.modes, got["ideal_actuators"], P)
    for e in range(B):
        assert abs(w2[e].std() - got["fit_rms"][e]) <= BOUND * got["rms"][e]
        assert np.linalg.norm(again["coef"][e]) <= BOUND * np.linalg.norm(got["coef"][e])


def test_abi_declares_and_exports_the_entry_points(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    for name in ("aog_upload_wavefront_fit", "aog_wavefront_truth"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
    assert re.search(r"#define AOG_ABI_VERSION\s+22\b", header) and _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert lib.aog_abi_version() == 22
    assert lib.aog_struct_size(9) == -1   # the feature adds no struct
    for name in ("aog_upload_wavefront_fit", "aog_wavefront_truth"):
        assert hasattr(lib, name), name


def test_null_handle_is_refused_without_a_gpu():
    lib = _lib.load()
    m = np.zeros(4)
    ptr = m.ctypes.data_as(ctypes.c_void_p)
    assert lib.aog_upload_wavefront_fit(None, ptr, ptr) == -1   # AOG_ERR_INVALID
    assert b"aog_upload_wavefront_fit" in lib.aog_last_error()
    assert lib.aog_wavefront_truth(None, ptr, ptr, ptr, ptr, None) == -1
    assert b"aog_wavefront_truth" in lib.aog_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(lib.aog_wavefront_truth(None, None, None, None, None, None))
