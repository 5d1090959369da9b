"""Layered atmosphere, host side (no GPU): the split of r0 over the layers, the layers' seeds, the argument checks, the C-ABI surface and
the self-consistency of the host restatement of ``aog_install_layer_sum`` (tests/layered_reference.py) that the GPU tests compare with."""
import os
import re

import numpy as np
import pytest

import layered_reference as ref
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.atmosphere_host import cn_squared_from_fried_parameter
from adaptive_optics_gym_amd.layered import MAX_LAYERS, layer_seed, resolve_layers


@pytest.mark.parametrize("fractions", [[1.0], [0.7, 0.3], [0.5, 0.3, 0.2]])
def test_fraction_split_conserves_cn_squared_per_env(fractions):
    wl = 2.2e-6
    r0 = np.array([0.08, 0.15, 0.31])
    plan = resolve_layers([{"fraction": f, "speed": 5.0 + i} for i, f in enumerate(fractions)], r0, 3)
    assert [p["fraction"] for p in plan] == fractions
    for e in range(3):
        total = sum(cn_squared_from_fried_parameter(float(p["fried"][e]), wl) for p in plan)
        np.testing.assert_allclose(total, cn_squared_from_fried_parameter(float(r0[e]), wl), rtol=1e-14)
    # a scalar r0 stays a scalar per layer; total_envs values are handed on whole (each layer's env slices them like atm_fried)
    plan = resolve_layers([{"fraction": 0.25, "speed": 3}, {"fraction": 0.75, "speed": [1, 2]}], 0.2, 2)
    assert isinstance(plan[0]["fried"], float) and plan[0]["fried"] == 0.2 * 0.25 ** (-3.0 / 5.0)
    plan = resolve_layers([{"fraction": 1.0, "speed": 3}], np.linspace(0.1, 0.2, 6), 2, total_envs=6, global_env_offset=2)
    assert plan[0]["fried"].shape == (6,)


def test_layer_seeds_are_distinct_and_layer_zero_keeps_the_envs_seed():
    for seed in (None, 0, 7, 1234, 2 ** 31 - 1):
        seeds = [layer_seed(seed, i) for i in range(MAX_LAYERS)]
        assert seeds[0] is seed or seeds[0] == seed
        rest = seeds[1:]
        assert len(set(rest)) == len(rest) and all(isinstance(s, int) and 0 <= s < 2 ** 31 for s in rest)
        assert (1234 if seed is None else seed) not in rest
        assert rest == [layer_seed(seed, i) for i in range(1, MAX_LAYERS)]   # a function of (seed, l) alone
    assert layer_seed(None, 3) == layer_seed(1234, 3) and layer_seed(7, 1) != layer_seed(8, 1)


@pytest.mark.parametrize("layers,fried,msg", [
    (None, 0.15, "atm_layers"),
    ([], 0.15, "atm_layers"),
    ([{"fraction": 1.0 / 9, "speed": 1}] * 9, 0.15, "atm_layers"),
    ({"fraction": 1.0, "speed": 1}, 0.15, "atm_layers"),
    ([{"fraction": 1.0}], 0.15, "keys"),
    ([{"fraction": 1.0, "speed": 1, "direction": 0.0}], 0.15, "keys"),
    ([{"fraction": 0.6, "speed": 1}, {"fraction": 0.3, "speed": 1}], 0.15, "sum to 1"),
    ([{"fraction": 0.5, "speed": 1}, {"fraction": 0.5 + 1e-9, "speed": 1}], 0.15, "sum to 1"),
    ([{"fraction": 1.2, "speed": 1}, {"fraction": -0.2, "speed": 1}], 0.15, "positive"),
    ([{"fraction": 0.0, "speed": 1}, {"fraction": 1.0, "speed": 1}], 0.15, "positive"),
    ([{"fraction": float("nan"), "speed": 1}], 0.15, "positive"),
    ([{"fraction": 1.0, "speed": -1}], 0.15, "atm_vel"),
    ([{"fraction": 1.0, "speed": float("inf")}], 0.15, "atm_vel"),
    ([{"fraction": 1.0, "speed": [1, 2, 3]}], 0.15, "atm_vel"),
    ([{"fraction": 1.0, "speed": 1}], -0.1, "atm_fried"),
    ([{"fraction": 1.0, "speed": 1}], [0.1, 0.2, 0.3], "atm_fried"),
])
def test_bad_layer_arguments_raise_value_error(layers, fried, msg):
    with pytest.raises(ValueError, match=msg):
        resolve_layers(layers, fried, 2)


def test_bad_arguments_raise_before_anything_is_created(monkeypatch):
    """LayeredAOEnv checks its layers before the parent constructor runs: no library, no device, no handle is touched."""
    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    def boom(self, *a, **k):
        raise AssertionError("the parent constructor ran")

    monkeypatch.setattr(BatchedAOEnv, "__init__", boom)
    for kw in (dict(atm_layers=[{"fraction": 0.5, "speed": 1}]), dict(atm_layers=[{"fraction": 1.0, "speed": -3}]), dict(atm_layers=None),
               dict(atm_layers=[{"fraction": 1.0, "speed": 1}], atm_type="quasi_static"),
               dict(atm_layers=[{"fraction": 1.0, "speed": 1}], atm_vel=3), dict(atm_layers=[{"fraction": 1.0, "speed": 1}], screens=np.zeros((2, 4, 4)))):
        with pytest.raises(ValueError):
            LayeredAOEnv(2, **kw)


def test_cabi_surface_lists_the_new_entry_points(repo_root):
    """Both entry points are declared, bound and exported, and header, binding and library agree on the ABI version.  (The version stays
    the one the other suites pin: the two calls are additions — no struct, constant or existing signature changed.)"""
    header = open(os.path.join(repo_root, "include", "aogym.h")).read()
    lib = _lib.load()
    for name in ("aog_evolve_atmosphere", "aog_install_layer_sum"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define AOG_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, header) and lib.aog_abi_version() == _lib.ABI_VERSION
    # argument checks that need no device
    assert lib.aog_evolve_atmosphere(None, None) == -1 and b"aog_evolve_atmosphere" in lib.aog_last_error()
    assert lib.aog_install_layer_sum(None, None, 1, None) == -1 and b"aog_install_layer_sum" in lib.aog_last_error()
    assert "layers" in __import__("adaptive_optics_gym_amd.build", fromlist=["UNITS"]).UNITS


def _case(N=12, B=5, L=3, seed=3):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:N, :N]
    ap_index = np.flatnonzero(((yy - (N - 1) / 2) ** 2 + (xx - (N - 1) / 2) ** 2 <= (N / 2) ** 2).ravel()).astype(np.int32)
    masters = [rng.randn(B, N, N) * 1e-6 * (l + 1) for l in range(L)]
    # origins: 0, N - 1, shifts of mixed signs taken mod N, per layer and per axis
    origins = [np.array([[0, 0], [N - 1, N - 1], [N - 1, 0], [(+2) % N, (-3) % N], [(-5) % N, (+4) % N]])[(np.arange(B) + l) % 5] for l in range(L)]
    return N, B, ap_index, masters, origins


def test_host_restatement_sums_through_the_origins():
    N, B, ap_index, masters, origins = _case()
    s = ref.layer_sum(masters, origins, ap_index, N)
    # the same through the unrolled (logical) screens: logical[iy][ix] = ring[(iy + oy) % N][(ix + ox) % N]
    logical = [np.stack([np.roll(m[b], shift=(-int(o[b, 1]), -int(o[b, 0])), axis=(0, 1)) for b in range(B)]) for m, o in zip(masters, origins)]
    want = logical[0].reshape(B, -1)[:, ap_index]
    for lg in logical[1:]:
        want = want + lg.reshape(B, -1)[:, ap_index]
    np.testing.assert_array_equal(s, want)
    np.testing.assert_array_equal(s, ref.layer_sum(logical, [np.zeros((B, 2), dtype=int)] * len(logical), ap_index, N))
    # each axis wraps on its own and each layer through its own origin: moving one layer's origin moves that layer only
    o2 = [o.copy() for o in origins]
    o2[1][:, 0] = (o2[1][:, 0] + 1) % N
    s2 = ref.layer_sum(masters, o2, ap_index, N)
    one = ref.layer_sum([masters[1]], [o2[1]], ap_index, N) - ref.layer_sum([masters[1]], [origins[1]], ap_index, N)
    np.testing.assert_allclose(s2 - s, one, rtol=0, atol=4 * np.finfo(float).eps * np.abs(s).max())


def test_host_restatement_mean_scaling_and_tile_order():
    N, B, ap_index, masters, origins = _case(N=14, B=37, L=2)
    wl = 1.5e-6
    out = ref.install(masters, origins, ap_index, N, wl)
    n_ap = ap_index.size
    assert n_ap % 32 != 0   # the last pixel tile is partly padding
    smax = np.abs(out["s"]).max()
    assert np.abs(out["psi64"].sum(axis=1)).max() <= n_ap * 2.0 ** -52 * smax * n_ap ** 0.5
    np.testing.assert_array_equal(out["psi64"], out["s"] - out["mean"][:, None])
    np.testing.assert_array_equal(out["rev"], (out["psi64"] / (2 * np.pi * wl)).astype(np.float32))
    # a piston on one layer changes nothing but the mean
    shifted = ref.install([masters[0] + 3e-6, masters[1]], origins, ap_index, N, wl)
    np.testing.assert_allclose(shifted["psi64"], out["psi64"], rtol=0, atol=8 * np.finfo(float).eps * (smax + 3e-6))
    # tile order: the documented index, a bijection onto distinct slots, zeros everywhere else, and the way back
    n_ptiles = (n_ap + 31) // 32
    assert out["tiles"].size == 2 * n_ptiles * 1024   # 37 envs: Bp = 64, two env tiles
    assert ref.tile_index(0, 0, n_ptiles) == 0 and ref.tile_index(1, 0, n_ptiles) == 4 and ref.tile_index(0, 1, n_ptiles) == 1
    assert ref.tile_index(0, 4, n_ptiles) == 32 * 4 and ref.tile_index(0, 8, n_ptiles) == 256 and ref.tile_index(0, 32, n_ptiles) == 1024
    assert ref.tile_index(32, 0, n_ptiles) == n_ptiles * 1024 and ref.tile_index(36, n_ap - 1, n_ptiles) < out["tiles"].size
    idx = ref.tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)
    assert np.unique(idx).size == B * n_ap
    rev, pad_nonzero = ref.unpack_tiles(out["tiles"], B, n_ap)
    np.testing.assert_array_equal(rev, out["rev"])
    assert pad_nonzero == 0 and np.count_nonzero(out["tiles"]) == np.count_nonzero(out["rev"])
