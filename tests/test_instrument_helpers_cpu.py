"""The argument and ``out=`` helpers the off-step instruments' wrappers share (``BatchedAOEnv._f64_arg`` / ``_f64_out``), on CPU tensors and
a shell of an env with no handle."""
import re

import numpy as np
import pytest
import torch

from adaptive_optics_gym_amd.batched_env import BatchedAOEnv


def _shell():
    env = object.__new__(BatchedAOEnv)
    env._torch, env.device = torch, torch.device("cpu")
    return env


def test_f64_arg_converts_and_holds_the_shape():
    env = _shell()
    assert env._f64_arg(None, (3, 2), "who", "x") is None
    good = torch.arange(6, dtype=torch.float64).reshape(3, 2)
    assert env._f64_arg(good, (3, 2), "who", "x") is good
    # an input may be a list, numpy, another dtype or a strided view: it arrives as a contiguous float64 tensor on the env's device
    for x in (good.tolist(), good.numpy(), good.float(), good.int(), torch.arange(12, dtype=torch.float64).reshape(3, 4)[:, ::2],
              np.arange(6, dtype=np.float32).reshape(3, 2)):
        t = env._f64_arg(x, (3, 2), "who", "x")
        assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (3, 2) and t.device == env.device
    assert torch.equal(env._f64_arg(good.float(), (3, 2), "who", "x"), good)
    for bad in (torch.zeros(2, 3), torch.zeros(3), torch.zeros(3, 2, 1), [[0.0, 0.0]] * 2):
        got = tuple(torch.as_tensor(bad).shape)
        with pytest.raises(ValueError, match="^" + re.escape(f"pyramid_gradient: g_slopes must have shape (3, 2), got {got}") + "$"):
            env._f64_arg(bad, (3, 2), "pyramid_gradient", "g_slopes")


def test_f64_out_takes_only_what_the_library_can_write_into():
    env = _shell()
    good = torch.ones((3, 2), dtype=torch.float64)
    assert env._f64_out(good, (3, 2), "who", "no") is good
    new = env._f64_out(None, (3, 2), "who", "no")
    assert new.dtype == torch.float64 and tuple(new.shape) == (3, 2) and new.device == env.device and not new.any()
    raw = env._f64_out(None, [3, 2], "who", "no", zero=False)
    assert raw.dtype == torch.float64 and tuple(raw.shape) == (3, 2)
    text = "a contiguous float64 [B, 2 n_valid] tensor on the env's device"
    bad = dict(shape=torch.ones((2, 3), dtype=torch.float64), dtype=good.float(), strided=torch.ones((3, 4), dtype=torch.float64)[:, ::2],
               device=good.to("meta"), no_tensor=good.numpy(), missing=False)
    for why, t in bad.items():
        with pytest.raises(ValueError, match="^" + re.escape(f"pyramid_slopes(out=...): expected {text}") + "$"):
            env._f64_out(t, (3, 2), "pyramid_slopes", text)
