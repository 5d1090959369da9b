"""The predictive controller without a device: the recursion as specified learns (numpy restatement, tests/predictor_reference.py), its
warm-up and symmetry properties, the C-ABI exports and every argument refusal of aog_predictor_create."""
import ctypes as C
import math

import numpy as np
import pytest

from adaptive_optics_gym_amd import _lib
from predictor_reference import RLSReference, rel_diff, run, var1_sequence


def _rotation_sequence(A, T, seed=3):
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(A, A))[0]
    y = np.empty((T, 1, A))
    y[0, 0] = 1e-7 * rng.randn(A)
    for t in range(1, T):
        y[t, 0] = Q @ y[t - 1, 0]
    return y


def test_reference_learns_a_rotation():
    """y_{t+1} = Q y_t, A = 6, order 1, lam = 1: the prediction error falls below 1e-6 |y| within 4 n steps and beats persistence over
    steps 2 n .. 4 n."""
    A = n = 6
    ys = _rotation_sequence(A, 4 * n + 1)
    # (lam = 1 keeps the prior P^-1 = I / p0 in the normal equations for ever: it biases the weights by about 1 / p0 against regressors of
    # unit size, so a prediction good to 1e-6 needs a weak prior)
    ref = RLSReference(1, A, 1, 1.0, 1e10, 1e-7)
    pred, _ = run(ref, ys[:-1])
    err = np.linalg.norm(pred[:, 0] - ys[1:, 0], axis=1)           # |pred_t - y_{t+1}|
    pers = np.linalg.norm(ys[1:, 0] - ys[:-1, 0], axis=1)
    norm = np.linalg.norm(ys[1:, 0], axis=1)
    print("relative prediction error per step:", err / norm)
    assert (err / norm).min() < 1e-6 and err[-1] / norm[-1] < 1e-6
    assert np.all(err[2 * n:] < pers[2 * n:])


@pytest.mark.parametrize("order", [1, 2, 3])
def test_first_predictions_are_the_measurements(order):
    ys = var1_sequence(5, order + 3, 2, 4)
    for dt in (np.float64, np.longdouble):
        ref = RLSReference(2, 4, order, 0.999, 1e3, 1.5e-6 / (2 * math.pi), dt)
        pred, innov = run(ref, ys)
        assert np.array_equal(pred[:order].astype(np.float64), ys[:order])
        assert not np.any(innov[:order])
        assert not np.array_equal(pred[order].astype(np.float64), ys[order]) and np.any(innov[order])
        assert np.all(ref.count == order + 3)


def test_p_stays_exactly_symmetric():
    ys = var1_sequence(11, 60, 2, 7)
    for ds in (False, True):
        ref = RLSReference(2, 7, 2, 0.99, 1e3, 2e-7, np.float64, ds)
        for y in ys:
            ref.update(y)
            assert np.array_equal(ref.P, ref.P.transpose(0, 2, 1))


def test_non_finite_rows_and_masks_in_the_reference():
    ys = var1_sequence(2, 8, 3, 4)
    ref = RLSReference(3, 4, 1, 0.999, 1e3, 2e-7)
    twin = RLSReference(3, 4, 1, 0.999, 1e3, 2e-7)
    for t, y in enumerate(ys):
        if t == 4:
            bad = y.copy()
            bad[1, 2] = np.nan
            W, P, h = ref.W.copy(), ref.P.copy(), ref.hist.copy()
            pred, innov = ref.update(bad)
            assert np.array_equal(pred[1], bad[1], equal_nan=True) and not np.any(innov[1])
            assert np.array_equal(ref.W[1], W[1]) and np.array_equal(ref.P[1], P[1]) and np.array_equal(ref.hist[1], h[1])
            assert list(ref.skipped) == [0, 1, 0] and list(ref.count) == [5, 4, 5]
            twin.update(y, mask=[True, False, True])
        else:
            ref.update(y)
            twin.update(y)
    assert np.array_equal(ref.W, twin.W) and np.array_equal(ref.P, twin.P)


def test_device_summation_order_stays_inside_the_envelope():
    """The kernel's summation order, emulated in float64, differs from the plain float64 recursion by less than 8 x the float64-versus-
    longdouble envelope: the bound tests/test_gpu_predictor.py holds the device to is one its own order of sums can meet."""
    B, A, p = 2, 33, 2
    ys = var1_sequence(166, 3 * A * p + 10, B, A)
    res = {}
    for name, dt, ds in (("f64", np.float64, False), ("ld", np.longdouble, False), ("dev", np.float64, True)):
        ref = RLSReference(B, A, p, 0.999, 1e3, 1.5e-6 / (2 * math.pi), dt, ds)
        res[name] = run(ref, ys) + (ref.W, ref.P)
    for k, what in enumerate(("pred", "innov", "W", "P")):
        env, dev = rel_diff(res["f64"][k], res["ld"][k]), rel_diff(res["dev"][k], res["f64"][k])
        print(f"{what}: envelope {env:.3e}, device order {dev:.3e}")
        assert env < 1e-6 and dev <= 8 * env


PRED_SYMBOLS = ("aog_predictor_create", "aog_predictor_destroy", "aog_predictor_reset", "aog_predictor_update", "aog_predictor_state_bytes",
                "aog_predictor_get_state", "aog_predictor_set_state")


def test_cabi_exports_the_predictor():
    lib = _lib.load()
    for name in PRED_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_lib.AogPredictorConfig) == 6 * 4 + 3 * 8


def _create(**kw):
    cfg = dict(batch=2, act_dim=8, order=2, env_id_base=0, reserved0=0, reserved1=0, forgetting=0.999, p0=1e3, scale=2e-7)
    cfg.update(kw)
    c = _lib.AogPredictorConfig(*[cfg[k] for k in ("batch", "act_dim", "order", "env_id_base", "reserved0", "reserved1", "forgetting", "p0", "scale")])
    h = C.c_void_p()
    lib = _lib.load()
    rc = lib.aog_predictor_create(C.byref(c), 0, C.byref(h))
    return rc, lib.aog_last_error().decode(), h


@pytest.mark.parametrize("kw", [dict(forgetting=0.0), dict(forgetting=-0.5), dict(forgetting=1.0000001), dict(forgetting=float("nan")),
                                dict(p0=0.0), dict(p0=-1.0), dict(p0=float("inf")), dict(p0=float("nan")),
                                dict(scale=0.0), dict(scale=-2e-7), dict(scale=float("inf")), dict(scale=float("nan")),
                                dict(reserved0=1), dict(reserved1=7), dict(order=0), dict(act_dim=0), dict(act_dim=257, order=1), dict(batch=0)])
def test_create_refuses_bad_arguments_before_any_device_work(kw):
    rc, msg, h = _create(**kw)
    assert rc == -1 and not h.value, (rc, msg)
    assert "aog_predictor_create" in msg


@pytest.mark.parametrize("A,order", [(64, 5), (256, 2), (129, 2), (1, 257)])
def test_create_names_the_sizes_it_does_not_support(A, order):
    rc, msg, h = _create(act_dim=A, order=order)
    assert rc == -4 and not h.value
    assert str(A) in msg and str(order) in msg and str(A * order) in msg and "256" in msg


def test_null_arguments_are_refused():
    lib = _lib.load()
    assert lib.aog_predictor_create(None, 0, None) == -1
    assert lib.aog_predictor_update(None, None, None, None, None, None) == -1
    assert lib.aog_predictor_reset(None, None, None) == -1
    assert lib.aog_predictor_get_state(None, None, None) == -1 and lib.aog_predictor_set_state(None, None, None) == -1
    assert lib.aog_predictor_state_bytes(None) == 0
    lib.aog_predictor_destroy(None)


def test_controller_argument_checks_need_no_device():
    from adaptive_optics_gym_amd.predictor import PredictiveController
    from adaptive_optics_gym_amd.rollout import rollout

    class Env:
        num_envs, num_modes, wavelength_wfs, pyramid, SH_operation, max_steps, device = 2, 4, 1.5e-6, None, True, 3, "cpu"

    with pytest.raises(ValueError, match="measurement"):
        PredictiveController(Env(), measurement="shack")
    with pytest.raises(ValueError, match="pyramid=dict"):
        PredictiveController(Env(), measurement="pyramid")
    with pytest.raises(ValueError, match="order"):
        PredictiveController(Env(), order=0)
    with pytest.raises(ValueError, match="forgetting"):
        PredictiveController(Env(), forgetting=1.5)
    with pytest.raises(ValueError, match="p0 and scale"):
        PredictiveController(Env(), scale=0.0)
    with pytest.raises(ValueError, match="predictor=PredictiveController"):
        rollout(Env(), None, policy="predictive")
    with pytest.raises(ValueError, match="predictor=PredictiveController"):
        rollout(Env(), None, policy="ideal", predictor=object())
