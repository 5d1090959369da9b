"""The life the six stand-alone handles share (csrc/standalone_handle.h), without a device: destroy and state_bytes of NULL, create's
null and config refusals, and every other entry point's null checks by the parameter names of include/.  Every refusal comes before any
device work — that this file passes on a machine without a GPU is the demonstration — and before the handle is looked at: the handle
the calls get is a block of zeros."""
import ctypes as C
import os
import re

import pytest

from adaptive_optics_gym_amd import _lib

INVALID, UNSUPPORTED = -1, -4   # AOG_ERR_INVALID, AOG_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")

# prefix -> (a good config, [(what to change, the return code, the field aog_last_error names)])
CONFIGS = {
    "aog_predictor": (dict(batch=2, act_dim=8, order=2, env_id_base=0, reserved0=0, reserved1=0, forgetting=0.999, p0=1e3, scale=2e-7),
                      [(dict(batch=0), INVALID, "batch"), (dict(act_dim=0), INVALID, "act_dim"), (dict(act_dim=257, order=1), INVALID, "act_dim"),
                       (dict(order=0), INVALID, "order"), (dict(reserved0=1), INVALID, "reserved"), (dict(reserved1=7), INVALID, "reserved"),
                       (dict(forgetting=0.0), INVALID, "forgetting"), (dict(forgetting=1.0000001), INVALID, "forgetting"),
                       (dict(forgetting=NAN), INVALID, "forgetting"), (dict(p0=0.0), INVALID, "p0"), (dict(p0=INF), INVALID, "p0"),
                       (dict(p0=NAN), INVALID, "p0"), (dict(scale=-2e-7), INVALID, "scale"), (dict(scale=INF), INVALID, "scale"),
                       (dict(scale=NAN), INVALID, "scale"), (dict(act_dim=64, order=5), UNSUPPORTED, "order"),
                       (dict(act_dim=129, order=2), UNSUPPORTED, "act_dim")]),
    "aog_telemetry": (dict(batch=2, act_dim=8, length=64, env_id_base=0),
                      [(dict(batch=0), INVALID, "batch"), (dict(act_dim=0), INVALID, "act_dim"), (dict(act_dim=129), INVALID, "act_dim"),
                       (dict(length=32), INVALID, "length"), (dict(length=2048), INVALID, "length"), (dict(length=96), INVALID, "length")]),
    "aog_spgd": (dict(abi_version=22, num_envs=2, act_dim=4, env_id_base=0, seed=1, metric=0, reserved0=0, clip=0.0),
                 [(dict(abi_version=21), INVALID, "abi_version"), (dict(num_envs=0), INVALID, "num_envs"), (dict(act_dim=0), INVALID, "act_dim"),
                  (dict(metric=3), INVALID, "metric"), (dict(metric=-1), INVALID, "metric"), (dict(reserved0=1), INVALID, "reserved"),
                  (dict(clip=-1.0), INVALID, "clip"), (dict(clip=NAN), INVALID, "clip"), (dict(clip=INF), INVALID, "clip")]),
    "aog_link": (dict(abi_version=22, num_envs=2, length=64, env_id_base=0, reserved=0),
                 [(dict(abi_version=21), INVALID, "abi_version"), (dict(num_envs=0), INVALID, "num_envs"), (dict(num_envs=-3), INVALID, "num_envs"),
                  (dict(length=32), INVALID, "length"), (dict(length=8192), INVALID, "length"), (dict(length=96), INVALID, "length"),
                  (dict(length=0), INVALID, "length"), (dict(reserved=1), INVALID, "reserved")]),
    "aog_disturbance": (dict(abi_version=22, num_envs=4, n_terms=2, env_id_base=0, seed=1),
                        [(dict(abi_version=21), INVALID, "abi_version"), (dict(num_envs=0), INVALID, "num_envs"), (dict(n_terms=0), INVALID, "n_terms"),
                         (dict(n_terms=9), INVALID, "n_terms")]),
    "aog_servo": (dict(abi_version=22, num_envs=4, act_dim=2, max_latency=1),
                  [(dict(abi_version=21), INVALID, "abi_version"), (dict(num_envs=0), INVALID, "num_envs"), (dict(act_dim=0), INVALID, "act_dim"),
                   (dict(act_dim=129), INVALID, "act_dim"), (dict(max_latency=-1), INVALID, "max_latency"), (dict(max_latency=5), INVALID, "max_latency"),
                   (dict(num_envs=2 ** 30, act_dim=128, max_latency=4), INVALID, "num_envs")]),
}
PREFIXES = tuple(CONFIGS)

# every other entry point with pointers it requires -> their positions (masks, the stream and the optional outputs are nullable)
REQUIRED = {
    "aog_predictor_reset": (0,), "aog_predictor_update": (0, 1, 3), "aog_predictor_get_state": (0, 1), "aog_predictor_set_state": (0, 1),
    "aog_telemetry_reset": (0,), "aog_telemetry_push": (0, 1), "aog_telemetry_psd": (0, 2), "aog_telemetry_gains": (0, 3, 5, 6),
    "aog_telemetry_get_state": (0, 1), "aog_telemetry_set_state": (0, 1),
    "aog_spgd_set_params": (0, 1, 2), "aog_spgd_reset": (0,), "aog_spgd_update": (0, 1, 3), "aog_spgd_get_state": (0, 1), "aog_spgd_set_state": (0, 1),
    "aog_link_reset": (0,), "aog_link_push": (0, 1), "aog_link_statistics": (0, 9, 10, 11, 12, 13, 14, 18), "aog_link_get_state": (0, 1),
    "aog_link_set_state": (0, 1),
    "aog_disturbance_set_params": (0, 1, 2, 3, 4, 5, 6), "aog_disturbance_reset": (0,), "aog_disturbance_advance": (0, 2),
    "aog_disturbance_coefficients": (0, 1), "aog_disturbance_get_state": (0, 1), "aog_disturbance_set_state": (0, 1),
    "aog_servo_set_params": (0, 1, 2, 3, 4, 5), "aog_servo_reset": (0,), "aog_servo_apply": (0, 1, 3), "aog_servo_get_state": (0, 1),
    "aog_servo_set_state": (0, 1),
}
LIFECYCLE = ("_create", "_destroy", "_state_bytes")


def _symbols():
    return {**_lib.SYMBOLS, **_lib.DISTURBANCE_SYMBOLS, **_lib.SERVO_SYMBOLS}


@pytest.fixture(scope="module")
def parameter_names(repo_root):
    """entry point -> its parameter names, as the headers under include/ write them"""
    text = "".join(open(os.path.join(repo_root, "include", h)).read() for h in ("aogym.h", "aogym_disturbance.h", "aogym_servo.h"))
    names = {}
    for name in REQUIRED:
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")
        names[name] = [re.findall(r"\w+", p)[-1] for p in params]
    return names


def _dummies(argtypes):
    """one non-null argument per position; `keep` holds what the pointers point at (zeros)"""
    keep, args = [], []
    for t in argtypes:
        if t is C.c_void_p:
            keep.append(C.create_string_buffer(4096))
            args.append(C.c_void_p(C.addressof(keep[-1])))
        elif t is C.c_int or t is C.c_double:
            args.append(t(1))
        else:   # POINTER(c_double): a host array
            keep.append((C.c_double * 64)())
            args.append(keep[-1])
    return keep, args


def test_every_entry_point_of_the_six_handles_is_covered():
    bound = {n for n in _symbols() if n.startswith(PREFIXES) and not n.endswith("_config_size")}
    assert bound == set(REQUIRED) | {p + s for p in PREFIXES for s in LIFECYCLE}
    assert set(_lib.STANDALONE) == set(PREFIXES)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_destroy_and_state_bytes_of_null(prefix):
    lib = _lib.load()
    assert getattr(lib, prefix + "_destroy")(None) is None
    assert getattr(lib, prefix + "_state_bytes")(None) == 0


@pytest.mark.parametrize("prefix", PREFIXES)
def test_create_names_its_null_argument(prefix):
    lib = _lib.load()
    create, cfg, out = getattr(lib, prefix + "_create"), _lib.STANDALONE[prefix][0](**CONFIGS[prefix][0]), C.c_void_p(0x5A5A)
    assert create(None, 0, C.byref(out)) == INVALID and lib.aog_last_error().decode().endswith(prefix + "_create: null argument cfg")
    assert out.value == 0x5A5A   # (nothing is written through `out` before the checks are through)
    assert create(C.byref(cfg), 0, None) == INVALID and lib.aog_last_error().decode().endswith(prefix + "_create: null argument out")
    assert create(None, 0, None) == INVALID and lib.aog_last_error().decode().endswith(prefix + "_create: null argument cfg")


@pytest.mark.parametrize("prefix,change,code,field", [(p, c, rc, f) for p, (_, cases) in CONFIGS.items() for c, rc, f in cases],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_create_refuses_a_bad_config_naming_the_field(prefix, change, code, field):
    lib = _lib.load()
    cfg, out = _lib.STANDALONE[prefix][0](**{**CONFIGS[prefix][0], **change}), C.c_void_p(0x5A5A)
    assert getattr(lib, prefix + "_create")(C.byref(cfg), 0, C.byref(out)) == code
    message = lib.aog_last_error().decode()
    assert prefix + "_create" in message and field in message, message
    assert not out.value


@pytest.mark.parametrize("name,position", [(n, p) for n, ps in REQUIRED.items() for p in ps])
def test_a_null_argument_is_named_before_anything_is_dereferenced(name, position, parameter_names):
    lib = _lib.load()
    keep, args = _dummies(_symbols()[name][1])
    args[position] = None
    assert getattr(lib, name)(*args) == INVALID
    assert lib.aog_last_error().decode().endswith(f"{name}: null argument {parameter_names[name][position]}")


def test_several_nulls_name_the_first_in_the_parameter_list(parameter_names):
    lib = _lib.load()
    for name, positions in REQUIRED.items():
        keep, args = _dummies(_symbols()[name][1])
        for p in positions:
            args[p] = None
        assert getattr(lib, name)(*args) == INVALID
        assert lib.aog_last_error().decode().endswith(f"{name}: null argument {parameter_names[name][positions[0]]}"), name


@pytest.mark.parametrize("position", [3, 5, 7, 15, 16, 17, 19])
def test_link_statistics_names_the_arrays_its_counts_ask_for(position, parameter_names):
    """edges_rel, hist_edges_rel and q with a count above 0; below, fades and longest with n_edges > 0; ber with n_q > 0"""
    lib = _lib.load()
    keep, args = _dummies(_symbols()["aog_link_statistics"][1])
    for p in (3, 5, 7):
        args[p][0] = 0.5   # (one positive factor each)
    args[position] = None
    assert lib.aog_link_statistics(*args) == INVALID
    assert lib.aog_last_error().decode().endswith("aog_link_statistics: null argument " + parameter_names["aog_link_statistics"][position])
