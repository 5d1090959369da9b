"""The analytic gradient of observation, power and Strehl, the parts that need no GPU: the numpy restatement tests/gradient_reference.py
against the CPU oracle (its forward) and against central finite differences of itself (its gradient), the scale invariance of the
outputs in the action, and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import gradient_reference as gr
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.optics_host import build_tables
from adaptive_optics_gym_amd.params import OpticalParams
from helpers import actions_for, run_oracle, smooth_screens

N, B = 32, 2
SHAPES = {"zernike6_o2": ("zernike", 6, 2), "disk20_o5": ("num_actuators", 20, 5)}
_TABLES = {}


def _tables(shape):
    if shape not in _TABLES:
        act_type, A, o = SHAPES[shape]
        _TABLES[shape] = build_tables(OpticalParams(num_pupil_pixels=N), act_type, A, o)
    return _TABLES[shape]


def _cotangents(n_obs, seed):
    """The rows the GPU tests use: one-hot centre and corner pixels, power alone, Strehl alone, a random mix."""
    rows = np.zeros((5, n_obs + 2))
    rows[0, n_obs // 2] = 1.0
    rows[1, 0] = 1.0
    rows[2, n_obs] = 1.0
    rows[3, n_obs + 1] = 1.0
    rows[4] = np.random.RandomState(seed).randn(n_obs + 2)
    return rows


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_forward_equals_the_oracle(shape):
    act_type, A, o = SHAPES[shape]
    t = _tables(shape)
    scr = smooth_screens(B, N, 21)
    actions = actions_for(B, A, 4)
    ref = run_oracle(scr, actions[None], act_type=act_type, act_dim=A, obs_dim=o)
    want = np.concatenate([ref["obs_raw"][0], ref["power"][0][:, None], ref["strehl"][0][:, None]], axis=1)
    got = gr.values_of(gr.phase(scr, gr.actuators_of_action(actions, t), t), t)
    err = np.abs(got - want) / np.abs(want)
    print(f"{shape}: reference forward against the oracle, max relative deviation {err.max():.2e}")
    assert got.shape == (B, o * o + 2)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_gradient_equals_finite_differences(shape):
    """Central differences of the reference forward in float64.  With step h in one coordinate x the two error terms, relative to the
    largest gradient component of the row, are
        truncation  ~ (d phi)^2 / 6, d phi the phase change of the step: (4 pi h / lambda_wfs)^2 / 6 for an actuator (|M| <= 1),
        round-off   ~ eps |L| / (h |grad|).
    h is chosen so that both are below a tenth of the bound 1e-5; the test computes and asserts both before it compares."""
    act_type, A, o = SHAPES[shape]
    t = _tables(shape)
    lam = t.params.wavelength_wfs
    bound, eps = 1e-5, np.finfo(np.float64).eps
    scr = smooth_screens(B, N, 22)
    action = actions_for(B, A, 5).astype(np.float64)
    act = gr.actuators_of_action(action, t)
    n_obs = o * o
    rows = _cotangents(n_obs, 9)
    val = gr.values_of(gr.phase(scr, act, t), t)

    def fd_jacobian(forward, x, h):
        J = np.empty((B, n_obs + 2, A))
        for k in range(A):
            d = np.zeros_like(x)
            d[:, k] = h
            J[:, :, k] = (forward(x + d) - forward(x - d)) / (2.0 * h)
        return J

    # with respect to the actuators
    h = 1e-10
    trunc = (4.0 * np.pi * h / lam) ** 2 / 6.0
    J = fd_jacobian(lambda a: gr.values_of(gr.phase(scr, a, t), t), act, h)
    for i, g in enumerate(rows):
        gbar = np.tile(g, (B, 1))
        an = gr.grad_actuators(scr, act, t, gbar)
        fd = np.einsum("ej,ejk->ek", gbar, J)
        scale = np.abs(an).max(axis=1)
        assert np.all(scale > 0)
        roundoff = eps * np.abs((gbar * val).sum(axis=1)) / (h * scale)
        err = np.abs(an - fd).max(axis=1) / scale
        print(f"{shape} cotangent {i}: d/d actuators  truncation {trunc:.1e}  round-off {roundoff.max():.1e}  deviation {err.max():.2e}")
        assert trunc <= bound / 10 and roundoff.max() <= bound / 10
        assert err.max() <= bound
    # with respect to the action: the step moves the actuators by at most c h / (10 n) per unit of v, a phase change of
    # d phi <= (4 pi / lambda_wfs) |a|_max h / |action|_min-ish; taken from the actuators' actual change
    ha = 1e-5
    dact = np.abs(gr.actuators_of_action(action + ha, t) - act).max() + np.abs(act).max() * ha / np.abs(action).min()
    trunc_a = (4.0 * np.pi * dact / lam) ** 2 / 6.0
    Ja = fd_jacobian(lambda a: gr.values_of(gr.phase(scr, gr.actuators_of_action(a, t), t), t), action, ha)
    for i, g in enumerate(rows):
        gbar = np.tile(g, (B, 1))
        an = gr.chain_to_action(gr.grad_actuators(scr, act, t, gbar), action, t)
        fd = np.einsum("ej,ejk->ek", gbar, Ja)
        scale = np.abs(an).max(axis=1)
        assert np.all(scale > 0)
        roundoff = eps * np.abs((gbar * val).sum(axis=1)) / (ha * scale)
        err = np.abs(an - fd).max(axis=1) / scale
        print(f"{shape} cotangent {i}: d/d action     truncation {trunc_a:.1e}  round-off {roundoff.max():.1e}  deviation {err.max():.2e}")
        assert trunc_a <= bound / 10 and roundoff.max() <= bound / 10
        assert err.max() <= bound
        # the outputs do not change with the action's scale (it is renormalised): action . grad = 0
        dot = np.abs(np.einsum("ek,ek->e", action, an))
        lim = 1e-10 * np.linalg.norm(action, axis=1) * np.linalg.norm(an, axis=1)
        print(f"{shape} cotangent {i}: |action . grad| / (|action| |grad|) = {(dot / lim * 1e-10).max():.2e}")
        assert np.all(dot <= lim)


def test_abi_declares_and_exports_the_entry_points(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    for name in ("aog_upload_gradient", "aog_output_gradient"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
    assert re.search(r"#define AOG_ABI_VERSION\s+22\b", header) and _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert lib.aog_abi_version() == 22
    for name in ("aog_upload_gradient", "aog_output_gradient"):
        assert hasattr(lib, name), name
    # the feature adds no struct: the sizes of the nine are what the bindings declare, and there is no tenth
    sizes = [lib.aog_struct_size(i) for i in range(9)]
    assert all(s > 0 for s in sizes) and lib.aog_struct_size(9) == -1
    assert sizes[0] == ctypes.sizeof(_lib.AogConfig) and sizes[1] == ctypes.sizeof(_lib.AogTables) and sizes[5] == ctypes.sizeof(_lib.AogInfo)


def test_null_handle_is_refused_without_a_gpu():
    lib = _lib.load()
    m = np.zeros(4)
    ptr = m.ctypes.data_as(ctypes.c_void_p)
    assert lib.aog_upload_gradient(None, ptr) == -1   # AOG_ERR_INVALID
    assert b"aog_upload_gradient" in lib.aog_last_error()
    assert lib.aog_output_gradient(None, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    assert b"aog_output_gradient" in lib.aog_last_error()
