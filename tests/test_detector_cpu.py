"""Photodetector model of the observations, host side: argument resolution (scalar / num_envs / total_envs values, slicing at the global env
offset, every refusal), the C surface (aog_set_detector declared, exported by the binding table, ABI still 22), and the host restatement
tests/detector_reference.py against scipy: the sampler's law on both branches, the stream's independence across env, pixel and frame."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import detector_reference as dr
from adaptive_optics_gym_amd import _lib
from adaptive_optics_gym_amd.params import resolve_detector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- resolve_detector ------------------------------------------------------------------------------------------------------------------------
def test_no_photons_means_no_detector():
    assert resolve_detector(None, 0.0, 0.0, 4, 4, 0) is None
    assert resolve_detector(None, 3.0, 1.0, 4, 8, 4) is None


def test_scalars_fill_every_env():
    d = resolve_detector(1e4, 2, None, 4, 4, 0)
    assert set(d) == {"photons", "read_noise", "background"}
    for k, v in (("photons", 1e4), ("read_noise", 2.0), ("background", 0.0)):
        assert d[k].dtype == np.float64 and d[k].flags.c_contiguous and np.array_equal(d[k], np.full(4, v))


def test_num_envs_and_total_envs_values_slice_at_the_offset():
    full = np.geomspace(10.0, 1e5, 10)
    local = resolve_detector(full[6:10], 1.0, 0.5, 4, 10, 6)
    assert np.array_equal(local["photons"], full[6:10])
    a = resolve_detector(full, np.arange(10.0), full / 100, 5, 10, 0)
    b = resolve_detector(full, np.arange(10.0), full / 100, 5, 10, 5)
    w = resolve_detector(full, np.arange(10.0), full / 100, 10, 10, 0)
    for k in w:
        assert np.array_equal(np.concatenate([a[k], b[k]]), w[k])
    assert np.array_equal(b["read_noise"], np.arange(5.0, 10.0))


@pytest.mark.parametrize("photons,read,back,match", [
    (0.0, 0, 0, "> 0"),
    (-5.0, 0, 0, "> 0"),
    (np.array([1e3, 0.0, 1e3]), 0, 0, "> 0"),
    (float("nan"), 0, 0, "finite"),
    (np.array([1e3, np.inf, 1e3]), 0, 0, "finite"),
    (np.array([1e3, 1e3]), 0, 0, "num_envs"),
    (np.ones((3, 1)), 0, 0, "num_envs"),
    (1e3, -1.0, 0, ">= 0"),
    (1e3, np.array([0.0, -1e-9, 0.0]), 0, ">= 0"),
    (1e3, float("nan"), 0, "finite"),
    (1e3, 0, -2.0, ">= 0"),
    (1e3, 0, np.array([0.0, 1.0, np.inf]), "finite"),
    (1e3, 0, np.zeros(4), "num_envs"),
    # a total_envs array is checked whole: the slices of a split batch refuse what the whole batch refuses
    (np.array([1e3, 1e3, 1e3, 1e3, 1e3, -1.0]), 0, 0, "> 0"),
])
def test_refusals(photons, read, back, match):
    with pytest.raises(ValueError, match=match):
        resolve_detector(photons, read, back, 3, 6, 0)


# ---- C surface -------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_and_bound_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "aogym.h")).read()
    assert re.search(r"int\s+aog_set_detector\s*\(\s*aog_env\s*\*\s*env\s*,\s*const\s+double\s*\*\s*photons_host\s*,\s*const\s+double\s*\*\s*read_noise_host\s*,"
                     r"\s*const\s+double\s*\*\s*background_host\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+AOG_ABI_VERSION\s+22\b", header)
    assert _lib.ABI_VERSION == 22
    res, args = _lib.SYMBOLS["aog_set_detector"]
    assert res is _lib.C.c_int and len(args) == 5
    host = open(os.path.join(ROOT, "adaptive_optics_gym_amd", "csrc", "aogym.hip")).read()
    assert re.search(r"^int aog_set_detector\(", host, re.M)


def test_library_exports_the_entry_point():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libaogym.so not built")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "aog_set_detector") and lib.aog_abi_version() == 22


def test_env_classes_take_the_keywords():
    import inspect

    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.envs.AO_env import AOEnv

    for cls in (BatchedAOEnv, AOEnv):
        p = inspect.signature(cls.__init__).parameters
        assert p["obs_photons"].default is None and p["obs_read_noise"].default == 0.0 and p["obs_background"].default == 0.0
    assert callable(BatchedAOEnv.set_detector) and isinstance(BatchedAOEnv.detector_parameters, property)


# ---- the restated stream ---------------------------------------------------------------------------------------------------------------------
def test_stream_words_are_keyed_by_env_pixel_frame_and_seed():
    base = dr.detector_words(64, np.arange(100, 164), 77, 5)
    assert base.shape == (64, 64, 4) and base.dtype == np.uint32
    assert np.array_equal(base, dr.detector_words(64, np.arange(100, 164), 77, 5))
    # a split batch draws what the whole one draws
    assert np.array_equal(base[32:], dr.detector_words(64, np.arange(132, 164), 77, 5))
    for other in (dr.detector_words(64, np.arange(101, 165), 77, 5), dr.detector_words(64, np.arange(100, 164), 78, 5),
                  dr.detector_words(64, np.arange(100, 164), 77 ^ (1 << 32), 5), dr.detector_words(64, np.arange(100, 164), 77, 6),
                  dr.detector_words(64, np.arange(100, 164), 77, 5 + (1 << 32)), dr.detector_words(64, np.arange(100, 164), 77, 5, tag=4)):
        assert np.mean(other == base) < 1e-3
    # env e + 1 at pixel j is not env e at pixel j + 1, nor frame f + 1 the neighbour env
    assert np.mean(base[1:, :-1] == base[:-1, 1:]) < 1e-3


def test_stream_is_independent_across_env_pixel_and_frame():
    """Uniforms of neighbouring envs, pixels and frames: lag-1 correlations within 5 / sqrt(M), and a uniformity chi-square."""
    w = np.stack([dr.detector_words(256, np.arange(7, 7 + 128), 1234, f) for f in range(8)])   # [frame, env, pixel, word]
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 - 0.5
    for axis in range(4):
        a, b = np.moveaxis(u, axis, 0)[1:], np.moveaxis(u, axis, 0)[:-1]
        r = float(np.mean(a * b) * 12.0)
        assert abs(r) <= 5.0 / np.sqrt(a.size), (axis, r)
    hist = np.bincount((w.ravel() >> np.uint32(24)).astype(np.int64), minlength=256)
    assert stats.chisquare(hist).pvalue > 1e-4


# ---- the restated sampler's law --------------------------------------------------------------------------------------------------------------
def _words(M, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 2 ** 32, size=(M, 4), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("lam", [0.02, 0.5, 3.0, 11.9])
def test_small_branch_is_poisson(lam):
    M = 400_000
    w = _words(M, 11)
    n, und = dr.poisson_small(np.full(M, lam), w[:, 0])
    assert und.mean() <= 1e-3
    kmax = int(n.max())
    obs = np.bincount(n.astype(np.int64), minlength=kmax + 1).astype(np.float64)
    exp = stats.poisson.pmf(np.arange(kmax + 1), lam) * M
    exp[-1] += stats.poisson.sf(kmax, lam) * M
    keep = exp >= 5
    obs_k, exp_k = np.append(obs[keep], obs[~keep].sum()), np.append(exp[keep], exp[~keep].sum())
    if exp_k[-1] < 5:
        obs_k, exp_k = np.append(obs_k[:-2], obs_k[-2:].sum()), np.append(exp_k[:-2], exp_k[-2:].sum())
    assert stats.chisquare(obs_k, exp_k * obs_k.sum() / exp_k.sum()).pvalue > 1e-4


@pytest.mark.parametrize("lam", [12.0, 150.0, 1e4])
def test_large_branch_matches_three_moments(lam):
    M = 1_000_000
    w = _words(M, 12)
    n, und = dr.poisson_large(np.full(M, lam), w[:, 0], w[:, 1])
    assert und.mean() <= 1e-3
    z = (n - lam) / np.sqrt(lam)
    # Poisson: mean lam, variance lam, third central moment lam; rounding adds 1/12 to the variance
    assert abs(z.mean()) <= 5.0 / np.sqrt(M)
    assert abs(z.var() - (1.0 + 1.0 / (12.0 * lam))) <= 5.0 * np.sqrt((2.0 + 1.0 / lam) / M) + 0.02 / lam
    skew_sd = np.sqrt(15.0 / M)    # sd of the sample third moment of a near-normal variable
    assert abs(np.mean(z ** 3) - 1.0 / np.sqrt(lam)) <= 5.0 * skew_sd + 0.05 / lam


def test_counts_switch_branches_at_12_and_frame_applies_the_model():
    B, n = 6, 40
    rs = np.random.RandomState(3)
    clean = rs.rand(B, n).astype(np.float32) * 0.2
    F = np.geomspace(5.0, 5e4, B)
    sig, back = np.full(B, 1.5), np.linspace(0.0, 3.0, B)
    fr = dr.frame(clean, F, sig, back, 10 + np.arange(B), 99, 3)
    w = dr.detector_words(n, 10 + np.arange(B), 99, 3)
    lam = F[:, None] * clean.astype(np.float64) + back[:, None]
    assert np.array_equal(fr["lam"], lam) and (lam < 12).any() and (lam >= 12).any()
    ns, _ = dr.poisson_small(np.where(lam < 12, lam, 0.0), w[..., 0])
    nl, _ = dr.poisson_large(np.where(lam < 12, 12.0, lam), w[..., 0], w[..., 1])
    assert np.array_equal(fr["n"], np.where(lam < 12, ns, nl))
    assert np.array_equal(fr["y"], (fr["n"] + sig[:, None] * dr.read_normal(w) - back[:, None]) / F[:, None])
    raw, half = dr.obs_of(fr["y"])
    assert raw.dtype == np.float32 and half.dtype == np.float16


def test_read_normal_is_standard_normal():
    w = _words(1_000_000, 13)
    g = dr.read_normal(w)
    assert abs(g.mean()) <= 5e-3 and abs(g.var() - 1.0) <= 8e-3
    assert stats.kstest(g[:200_000], "norm").pvalue > 1e-4
    # independent of the count's words
    gc = dr.normal24(w[:, 0], w[:, 1], np.float64)
    assert abs(np.mean(g * gc)) <= 5e-3


def test_host_rule_leaves_out_little():
    """The share of draws the host rule flags as undecidable, lam log-uniform over both branches: far below the 0.1 % the GPU tests allow."""
    M = 500_000
    w = _words(M, 14)
    rs = np.random.RandomState(15)
    lam_s, lam_l = np.exp(rs.uniform(np.log(0.02), np.log(12.0), M)), np.exp(rs.uniform(np.log(12.0), np.log(1e4), M))
    _, us = dr.poisson_small(lam_s, w[:, 0])
    _, ul = dr.poisson_large(lam_l, w[:, 0], w[:, 1])
    assert us.mean() <= 5e-4 and ul.mean() <= 5e-5
