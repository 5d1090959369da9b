"""The link telemetry without a device: the C-ABI surface, every argument refusal (they come before any handle exists), and the numpy
restatement (tests/link_reference.py) against a second formulation and against the kernel's own combination rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import link_reference as ref
from adaptive_optics_gym_amd import _lib

LINK_SYMBOLS = ("aog_link_create", "aog_link_destroy", "aog_link_reset", "aog_link_push", "aog_link_statistics", "aog_link_state_bytes",
                "aog_link_get_state", "aog_link_set_state")


def test_cabi_surface_lists_the_link_entry_points(repo_root):
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    lib = _lib.load()
    for name in LINK_SYMBOLS:
        assert re.search(r"\b(int|void|int64_t)\s+%s\s*\(" % name, header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define AOG_ABI_VERSION\s+22\b", header) and _lib.ABI_VERSION == 22 and lib.aog_abi_version() == 22
    assert C.sizeof(_lib.AogLinkConfig) == 20
    # argument checks that need no device
    stats = (None, 1, 0.0, None, 0, None, 0, None, 0) + (None,) * 13
    for name, args in (("aog_link_create", (None, 0, None)), ("aog_link_reset", (None,) * 3), ("aog_link_push", (None,) * 4), ("aog_link_statistics", stats),
                       ("aog_link_get_state", (None,) * 3), ("aog_link_set_state", (None,) * 3)):
        assert getattr(lib, name)(*args) == -1 and name.encode() in lib.aog_last_error(), name
    assert lib.aog_link_state_bytes(None) == 0
    lib.aog_link_destroy(None)
    assert "link" in __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"]).UNITS


@pytest.mark.parametrize("kw,field", [(dict(abi_version=21), "abi_version"), (dict(num_envs=0), "num_envs"), (dict(num_envs=-3), "num_envs"),
                                      (dict(length=32), "length"), (dict(length=8192), "length"), (dict(length=96), "length"), (dict(length=0), "length"),
                                      (dict(reserved=1), "reserved")])
def test_create_refuses_bad_configs_naming_the_field(kw, field):
    cfg = dict(abi_version=_lib.ABI_VERSION, num_envs=2, length=64, env_id_base=0, reserved=0)
    cfg.update(kw)
    h = C.c_void_p()
    lib = _lib.load()
    assert lib.aog_link_create(C.byref(_lib.AogLinkConfig(*cfg.values())), 0, C.byref(h)) == -1 and not h.value
    message = lib.aog_last_error().decode()
    assert "aog_link_create" in message and field in message, message


def test_link_telemetry_is_exported():
    import adaptive_optics_gym_amd as pkg
    from adaptive_optics_gym_amd import LinkTelemetry
    from adaptive_optics_gym_amd.link import LinkTelemetry as direct

    assert LinkTelemetry is direct and "LinkTelemetry" in pkg.__all__
    assert (direct.prefix, direct.noun, direct.lazy) == ("aog_link", "link telemetry", True)


def test_argument_errors_come_before_any_handle():
    from adaptive_optics_gym_amd.link import LinkTelemetry

    t = LinkTelemetry(2, length=64)
    for bad in ([-3, -6], [-6, -6], [-6, float("nan")], [float("inf")], np.linspace(-20, -1, 17), [[-3.0]]):
        with pytest.raises(ValueError, match="thresholds_db"):
            t.statistics(thresholds_db=bad)
    for bad in ([0, -1], [1.0, 1.0], [float("-inf"), 0.0], np.linspace(-30, 6, 65)):
        with pytest.raises(ValueError, match="hist_edges_db"):
            t.statistics(hist_edges_db=bad)
    for bad in ([0.0], [6.0, -1.0], [float("nan")], [float("inf")], np.linspace(1, 9, 9)):
        with pytest.raises(ValueError, match="q"):
            t.statistics(q=bad)
    for bad in (0.0, -1e-4, float("nan"), float("inf"), "median"):
        with pytest.raises(ValueError, match="reference"):
            t.statistics(reference=bad)
    good = torch.zeros(2, dtype=torch.float32)
    for bad in (good, good.double(), torch.zeros(3), torch.zeros(2, 1), torch.zeros(4)[::2], [0.0, 0.0], None):   # (a host tensor is not on the telemetry's device)
        with pytest.raises(ValueError, match="power"):
            t.push(bad)
    assert t._handle is None
    for length in (32, 100, 8192):
        with pytest.raises(ValueError, match="length"):
            LinkTelemetry(2, length=length)
    with pytest.raises(ValueError, match="num_envs"):
        LinkTelemetry(0)
    assert LinkTelemetry(5).length == 1024 and LinkTelemetry(5, 4096).state_bytes() == 5 * (4 * 4096 + 16)
    with pytest.raises(ValueError, match="length"):
        t.load_state_dict(dict(blob=None, num_envs=2, length=128))


# ---- the restatement against a second formulation -------------------------------------------------------------------------------------------
LOW, HIGH = 0.25, 1.0   # (exact in float32; the threshold sits at 0.5 of the absolute reference 1)
WINDOWS = {
    "all in fade": [LOW] * 9,
    "none in fade": [HIGH] * 9,
    "alternating": [LOW, HIGH] * 6,
    "a run at each end": [LOW, LOW, LOW, HIGH, HIGH, LOW, HIGH, HIGH, LOW, LOW],
    "one sample in fade": [LOW],
    "one sample out of fade": [HIGH],
    "empty": [],
}
EXPECTED = {"all in fade": (9, 1, 9), "none in fade": (0, 0, 0), "alternating": (6, 6, 1), "a run at each end": (6, 3, 3), "one sample in fade": (1, 1, 1),
            "one sample out of fade": (0, 0, 0), "empty": (0, 0, 0)}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_the_reference_agrees_with_the_brute_force_formulation(name):
    win = np.array(WINDOWS[name], dtype=np.float32)
    s = ref.statistics(win, 1.0, factors=[0.5, 2.0], hist_factors=[0.5, 2.0], q=[1.0, 4.0])
    in_fade = [float(v) < 0.5 for v in win]
    assert (s["below"][0], s["fades"][0], s["longest"][0]) == EXPECTED[name] == ref.runs_brute(in_fade) == ref.runs(in_fade)
    n = len(win)
    assert (s["below"][1], s["fades"][1], s["longest"][1]) == (n, min(n, 1), n)                  # everything lies below 2
    assert s["hist"] == ref.hist_brute(win, [0.5, 2.0]) and sum(s["hist"]) == n and s["samples"] == n
    if n == 0:
        assert all(np.isnan(s[k]) for k in ("mean", "mean_square", "scintillation_index", "minimum", "maximum", "reference")) and np.isnan(s["ber"]).all()
        return
    assert s["mean"] == float(np.mean(win.astype(np.float64))) and s["mean_square"] == float(np.mean(win.astype(np.float64) ** 2))   # (exact: dyadic values)
    assert s["minimum"] == win.min() and s["maximum"] == win.max()
    # Q = 4 at the reference level itself is the textbook 3.17e-5; the mean over the window follows from the two levels
    want = [np.mean([0.5 * ref.math.erfc(q * v / 2 ** 0.5) for v in win.astype(np.float64)]) for q in (1.0, 4.0)]
    np.testing.assert_allclose(s["ber"], want, rtol=1e-14)
    if name == "none in fade":
        assert abs(s["ber"][1] - 3.167124183e-5) < 1e-13
    m = ref.statistics(win, "mean", factors=[0.5])
    assert m["reference"] == m["mean"] and m["edges"] == [0.5 * m["mean"]]


def test_the_segment_merge_reproduces_the_loop_for_any_chunking():
    """What the kernel does — chunks reduced to summaries, merged in order by a tree — against the plain loop: random sequences of every
    fade density, runs longer than a chunk, and every chunk size the kernel uses."""
    rng = np.random.RandomState(11)
    for chunk in (1, 2, 16, 64):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            for n in (0, 1, chunk, 37 * chunk, 64 * chunk - 1, 64 * chunk):
                f = list(rng.rand(n) < density)
                assert ref.merged_runs(f, chunk) == ref.runs(f) == ref.runs_brute(f), (chunk, density, n)
    f = [False] * 4096
    for a, b in ((0, 5), (1000, 1200), (2048, 2058), (2105, 2112), (2560, 2624), (3130, 3140), (4090, 4096)):
        f[a:b] = [True] * (b - a)
    assert ref.merged_runs(f, 64) == (5 + 200 + 10 + 7 + 64 + 10 + 6, 7, 200)
    left, right, empty = ref.segment([True, False, True, True]), ref.segment([True, True, False]), ref.segment([])
    assert ref.merge(left, right) == ref.segment([True, False, True, True, True, True, False]) == (7, 5, 2, 1, 0, 4)
    assert ref.merge(left, empty) == left == ref.merge(empty, left)


def test_the_ring_restatement_wraps_skips_and_masks():
    ring = ref.RingReference(3, 8)
    for t in range(11):
        p = np.full(3, float(t), dtype=np.float32)
        if t == 4:
            p[1] = np.inf
        ring.push(p, mask=[True, True, t % 2 == 0])
    assert list(ring.count) == [11, 10, 6] and list(ring.skipped) == [0, 1, 0]
    assert list(ring.window(0)) == [3, 4, 5, 6, 7, 8, 9, 10] and list(ring.window(1)) == [2, 3, 5, 6, 7, 8, 9, 10] and list(ring.window(2)) == [0, 2, 4, 6, 8, 10]
    ring.reset([False, True, False])
    assert list(ring.count) == [11, 0, 6] and not ring.ring[1].any() and ring.window(1).size == 0


# ---- rollout(..., link=) ------------------------------------------------------------------------------------------------------------------
class _Env:
    """The BatchedAOEnv interface on CPU tensors, as tests/test_rollout_cpu.py's stand-in; a step would be a failure here."""

    def __init__(self, B, device="cpu"):
        self.num_envs, self.max_steps, self.device, self.resets = B, 3, torch.device(device), 0

    def reset(self):
        self.resets += 1
        return torch.zeros(self.num_envs, 4, dtype=torch.float16), {}

    def step(self, a):
        raise AssertionError("rollout stepped an env whose link it had to refuse")


def test_rollout_refuses_a_mismatched_link_before_the_first_step():
    from adaptive_optics_gym_amd import LinkTelemetry
    from adaptive_optics_gym_amd.rollout import make_actor, rollout

    actor = make_actor(4, 6, 8)
    env = _Env(3)
    with pytest.raises(ValueError, match="link holds 2 envs"):
        rollout(env, actor, link=LinkTelemetry(2, length=64))
    with pytest.raises(ValueError, match="link lives on"):          # the right size on another device
        rollout(env, actor, link=LinkTelemetry(3, length=64))
    with pytest.raises(ValueError, match="LinkTelemetry"):
        rollout(env, actor, link=object())
    assert env.resets == 0
