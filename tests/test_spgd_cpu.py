"""The SPGD controller without a device: the C-ABI surface, the argument refusals of rollout and SPGDController, the bit map of the numpy
restatement (tests/spgd_reference.py) and the closed form of one iteration on a quadratic metric."""
import ctypes as C
import itertools
import os
import re
import types

import numpy as np
import pytest

import spgd_reference as ref
from adaptive_optics_gym_amd import _lib

NEW_SYMBOLS = ("aog_spgd_create", "aog_spgd_destroy", "aog_spgd_set_params", "aog_spgd_reset", "aog_spgd_update", "aog_spgd_state_bytes",
               "aog_spgd_get_state", "aog_spgd_set_state", "aog_reset_spgd", "aog_step_spgd")


def test_header_declares_the_symbols_and_keeps_abi_22(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    assert re.search(r"#define AOG_ABI_VERSION\s+22\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
    m = re.search(r"typedef struct aog_spgd_config \{(.*?)\} aog_spgd_config;", header, re.S)
    assert m
    for field in ("abi_version", "num_envs", "act_dim", "env_id_base", "seed", "metric", "clip"):
        assert re.search(r"\b%s\b" % field, m.group(1)), field
    assert C.sizeof(_lib.AogSpgdConfig) == 4 * 4 + 8 + 2 * 4 + 8


def test_library_exports_the_symbols():
    lib = _lib.load()
    assert lib.aog_abi_version() == 22 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name


class _Env:
    num_envs, num_modes, SH_operation, max_steps, device, obs_dim, science_window = 2, 4, True, 3, "cpu", 2, (0, 1)

    def _base_seed(self):
        return 1234


def test_rollout_refuses_the_combinations_before_anything_runs():
    from adaptive_optics_gym_amd.rollout import OrnsteinUhlenbeckNoise, rollout

    env = _Env()
    ctrl = types.SimpleNamespace(env=env)   # (rollout must refuse before it touches the controller)
    with pytest.raises(ValueError, match="controller=SPGDController"):
        rollout(env, None, policy="spgd")
    with pytest.raises(ValueError, match="another env"):
        rollout(_Env(), None, policy="spgd", controller=ctrl)
    ou = OrnsteinUhlenbeckNoise(2, 4, 0.0, 0.3, 0.05)
    for kw in (dict(lookahead=True), dict(science=True), dict(ou_noise=ou), dict(action_mode="mean")):
        for fused in (False, True):
            with pytest.raises(ValueError, match="policy='spgd' goes with none of"):
                rollout(env, None, policy="spgd", controller=ctrl, fused_policy=fused, **kw)
    plain = _Env()
    plain.SH_operation = False
    with pytest.raises(ValueError, match="SH_operation=True"):
        rollout(plain, None, policy="spgd", controller=types.SimpleNamespace(env=plain))


def test_controller_refuses_bad_arguments_before_creating_anything():
    from adaptive_optics_gym_amd.sensorless import SPGDController

    plain = _Env()
    plain.SH_operation = False
    with pytest.raises(ValueError, match="SH_operation=True"):
        SPGDController(plain)
    env = _Env()
    with pytest.raises(ValueError, match="metric"):
        SPGDController(env, metric="ssim")
    for bad in (-1.0, float("nan"), float("inf"), [0.1, -0.1]):
        with pytest.raises(ValueError, match="gain"):
            SPGDController(env, gain=bad)
        with pytest.raises(ValueError, match="amplitude"):
            SPGDController(env, amplitude=bad)
    with pytest.raises(ValueError, match="gain"):
        SPGDController(env, gain=[0.1, 0.2, 0.3])   # B = 2
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip"):
            SPGDController(env, clip=bad)


def test_library_refuses_bad_configurations_without_a_device():
    lib = _lib.load()

    def create(**kw):
        f = dict(abi_version=22, num_envs=2, act_dim=4, env_id_base=0, seed=1, metric=0, reserved0=0, clip=0.0)
        f.update(kw)
        h = C.c_void_p()
        rc = lib.aog_spgd_create(C.byref(_lib.AogSpgdConfig(**f)), 0, C.byref(h))
        return rc, lib.aog_last_error().decode()

    for kw, text in ((dict(abi_version=21), "abi_version"), (dict(num_envs=0), "dimensions"), (dict(act_dim=0), "dimensions"), (dict(metric=3), "metric"),
                     (dict(metric=-1), "metric"), (dict(reserved0=1), "reserved"), (dict(clip=-1.0), "clip"), (dict(clip=float("nan")), "clip")):
        rc, msg = create(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    assert lib.aog_spgd_update(None, None, None, None, None) != 0 and "null" in lib.aog_last_error().decode()
    assert lib.aog_step_spgd(None, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert lib.aog_spgd_state_bytes(None) == 0


# ---- the reference's Philox bit map ----
@pytest.mark.parametrize("counter, key, expect", [
    # the Random123 known answers tests/test_actor_reference_cpu.py pins its own Philox with
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    assert " ".join("%08x" % w for w in ref.philox4x32_10(counter, key)) == expect


def test_bit_map_of_the_reference():
    seed, A = 0x1234567890ABCDEF, 200
    d3, d4 = ref.delta_bits(seed, 3, 7, A), ref.delta_bits(seed, 4, 7, A)
    assert d3.shape == (A,) and not np.array_equal(d3, d4)                       # two global env ids: two streams
    assert not np.array_equal(d3, ref.delta_bits(seed, 3, 8, A))                 # and every iteration its own
    assert not np.array_equal(d3, ref.delta_bits(seed ^ (1 << 32), 3, 7, A))     # the seed's high word is part of the key
    w0 = ref.philox4x32_10((3, 7, 0, ref.TAG), (seed & 0xFFFFFFFF, seed >> 32))
    w1 = ref.philox4x32_10((3, 7, 1, ref.TAG), (seed & 0xFFFFFFFF, seed >> 32))
    assert d3[31] == (w0[0] >> 31) & 1 and d3[32] == w0[1] & 1                   # 31 -> 32: the adjacent word
    assert d3[127] == (w0[3] >> 31) & 1 and d3[128] == w1[0] & 1                 # 127 -> 128: the next call
    assert d3[199] == (w1[2] >> 7) & 1
    for i in range(A):
        w = (w0, w1)[i >> 7][(i >> 5) & 3]
        assert d3[i] == (w >> (i & 31)) & 1
    # a shorter act_dim is a prefix: the map does not depend on A
    assert np.array_equal(ref.delta_bits(seed, 3, 7, 6), d3[:6])
    d = ref.delta(seed, 3, 7, A)
    assert set(np.unique(d)) == {-1.0, 1.0} and np.array_equal(d > 0, d3)
    assert 0.35 < d3.mean() < 0.65


def test_reference_state_machine_masks_and_reset():
    c = ref.SPGD(3, 5, [0.5, 1.0, 2.0], 0.1, seed=9, env_id_base=10)
    a0 = c.reset()
    assert np.array_equal(a0, np.where(np.stack([ref.delta_bits(9, 10 + b, 0, 5) for b in range(3)]), 0.1, -0.1).astype(np.float32))
    a1 = c.update(np.array([1, 2, 3], np.float32))
    assert np.array_equal(a1, -a0) and list(c.h) == [1, 1, 1] and list(c.J_plus) == [1, 2, 3] and not c.u.any()
    c.update(np.array([0.5, 2, 4], np.float32), mask=[True, False, True])
    assert list(c.k) == [1, 0, 1] and list(c.h) == [0, 1, 0]
    assert np.array_equal(c.u[0], 0.5 * 0.5 * ref.delta(9, 10, 0, 5)) and not c.u[1].any() and np.array_equal(c.u[2], 2.0 * -1.0 * ref.delta(9, 12, 0, 5))
    out = c.reset(mask=[False, False, True])
    assert list(c.k) == [1, 0, 1] and list(c.h) == [0, 1, 0] and not c.u[2].any() and c.u[0].any() and not out[:2].any()
    clipped = ref.SPGD(1, 5, 100.0, 0.1, seed=9, clip=0.25)
    clipped.reset()
    clipped.update(np.array([1], np.float32))
    clipped.update(np.array([0], np.float32))
    assert np.array_equal(np.abs(clipped.u), np.full((1, 5), 0.25))


# ---- closed form on a quadratic metric ----
def test_one_iteration_on_a_quadratic_metric():
    """J(a) = -|a - a*|^2: J_plus - J_minus = -4 amplitude delta'(u - a*) and, over all 2^A sign patterns, E[du] = -4 gain amplitude (u - a*)."""
    A, gain, amp = 4, 0.3, 0.05
    rng = np.random.RandomState(5)
    u, target = rng.randn(A), rng.randn(A)

    def J(a):
        return -np.sum((a - target) ** 2)

    mean_du = np.zeros(A)
    for signs in itertools.product((-1.0, 1.0), repeat=A):
        d = np.array(signs)
        diff = J(u + amp * d) - J(u - amp * d)
        assert abs(diff - (-4.0 * amp * d @ (u - target))) < 1e-12
        mean_du += gain * diff * d / 2 ** A
    assert np.max(np.abs(mean_du - (-4.0 * gain * amp * (u - target)))) < 1e-12
    # the same through the reference's own state machine, with its own delta (float64 J through a float32: exact here by construction)
    c = ref.SPGD(1, A, gain, amp, seed=77)
    c.u[0] = u32 = np.float32(u).astype(np.float64)
    d = ref.delta(77, 0, 0, A)
    Jp, Jm = np.float32(J(u32 + amp * d)), np.float32(J(u32 - amp * d))
    c.update(np.array([Jp]))
    c.update(np.array([Jm]))
    assert np.array_equal(c.u[0], u32 + gain * (np.float64(Jp) - np.float64(Jm)) * d) and c.k[0] == 1
