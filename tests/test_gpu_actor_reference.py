"""The policy query kernels (k_actor_act, k_actor_act_noise, the fused step tail: actor_mlp of csrc/k_actor.h) with dropout ON against a host
replay of their random streams (tests/actor_reference.py: Philox4x32-10 regenerated word for word, the masked network in float64).

Every B x A mean, action and OU state and every B log_prob of three consecutive calls per case is compared; nothing is masked out.

* mean: rtol 2e-5, atol 2e-6 x max(1, max |ref|) against the float64 reference with the exact masks (the project's tolerance of this kernel
  at dropout_p = 0).  Cases listed in actor_reference.F32_SPREAD_CASES would be held to 8 x the spread of a float32 numpy evaluation of the
  same masked network instead; none needs it (measured figures below).
* zero pattern (layers 2, 3 and the output layer identities): the exactly-zero means are the units the reference drops in any layer or whose
  pre-activation is below -1e-3, the nonzero ones the units kept three times with a pre-activation above 1e-3.
* eps = (action - mean) / sqrt(cov_var): 2.4e-5 (16 x the 1.5e-6 of a float32 numpy Box-Muller on the same words) + ulp32(|action|) / std,
  at most 1e-4; a query with zero output weights gives action = std eps and is held to 2.4e-5 alone.
* log_prob: rtol 1e-4, atol 1e-3.  Mean mode: action == mean bit for bit, log_prob == the float32 constant.
* OU: new state within sigma x 2.4e-5 of the float64 recursion on the reference's tag-5 normals (sigma = 0: equal), action ==
  float32(float64(plain action) + state) bit for bit, rows past the batch untouched.

Measured on an MI355X (largest fraction of each bound used over the three calls and both observation types; f32 spread = the largest
deviation of a float32 numpy evaluation of the same masked network from float64, of which 8 x would be the fallback allowance):

  case                      mean    eps     eps deviation  OU state  f32 spread
  reference_shape_ragged    0.10    0.029   7.1e-7         0.024     1.3e-6
  o5                        0.07    0.021   5.0e-7         0.017     7.2e-7
  one_tile_odd_one_env      0.005   0.002   4.5e-8         0.001     2.4e-8
  act_dim_6_p09             0.014   0.008   1.9e-7         0.013     9.9e-7
  weight_chunks_h400        0.12    0.023   5.7e-7         0.018     2.6e-6
  state_256_over_hidden     0.21    0.016   3.9e-7         0.014     1.1e-6
  separable_obs_1024        0.30    0.020   5.0e-7         0.014     1.6e-6
  hidden_496_beside_1024    0.24    0.017   4.1e-7         0.011     2.0e-6
  hidden_848_widest         0.12    0.019   4.5e-7         0.011     1.8e-6
  keying_fields             0.05    0.022   5.3e-7         0.015     6.3e-7
  p0_regression             0.07    0.023   5.6e-7         0.018     4.8e-7
  fused tail o = 2          0.09    0.022   5.3e-7         0.013
  fused tail o = 32         0.03    0.023   5.7e-7         0.016

Every case meets the rtol / atol bound on the mean, so F32_SPREAD_CASES is empty.  The identity construction's means use at most 0.15 of
theirs.  Hardware Box-Muller (v_log_f32, v_sqrt_f32, v_cos_f32 / v_sin_f32) against float64 on the same float32 uniforms, read off without
the recovery rounding (test_eps_without_recovery, 192 000 normals, |eps| up to 4.5): 5.7e-7, 0.024 of the 2.4e-5 allowed.  log_prob uses
at most 0.002 of its bound.  In one_tile_odd_one_env and act_dim_6_p09 the identity construction leaves every mean zero (one unit kept
with probability 1/8; 30 units with probability 1e-3): there the pattern only says that nothing survives which the reference drops.
"""
import ctypes as C

import numpy as np
import pytest

import actor_reference as ar
from helpers import smooth_screens

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in ar.CASES]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _module(weights):
    """make_actor's module on the GPU holding ``weights`` (w1, b1, ..., wo, bo)."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import make_actor

    H, S = weights[0].shape
    actor = make_actor(S, weights[6].shape[0], H, device="cuda:0")
    with torch.no_grad():
        for i, layer in enumerate(list(actor.hidden) + [actor.out]):
            layer.weight.copy_(torch.from_numpy(weights[2 * i]))
            layer.bias.copy_(torch.from_numpy(weights[2 * i + 1]))
    return actor


def _device_actor(actor, case, call):
    from adaptive_optics_gym_amd.rollout import DeviceActor

    da = DeviceActor(actor, seed=case.seed, dropout_p=case.p, env_id_base=case.env_id_base)
    da.calls = case.call_index + call
    return da


def _np(tensors):
    return [t.detach().cpu().numpy().copy() for t in tensors]


def _logp_const(A, cov_var):
    """The host's float32 constant 0.5 A log(2 pi cov_var) (actor_args: float arithmetic, libm's logf)."""
    logf = C.CDLL("libm.so.6").logf
    logf.restype, logf.argtypes = C.c_float, [C.c_float]
    f = np.float32
    return f(f(0.5) * f(A)) * f(logf(float(f(2.0) * f(np.pi) * f(cov_var))))


def _report(record_property, log, **extra):
    """The largest fraction of each bound a test used, as properties of the test and on its output."""
    worst = {}
    for what, figures in log:
        kind = what.split(":")[0]
        for k, v in figures.items():
            worst[f"{kind}.{k}"] = max(worst.get(f"{kind}.{k}", 0.0), v)
    worst.update(extra)
    for k, v in sorted(worst.items()):
        record_property(k, v)
    print("ACTOR_REFERENCE " + " ".join(f"{k}={v:.4g}" for k, v in sorted(worst.items())))


def _ou(B, A, sigma, start, extra_rows=3):
    """A DeviceOUNoise whose state is the first B rows of an over-allocated block; the rows past B hold a sentinel."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceOUNoise

    ou = DeviceOUNoise(B, A, mu=ar.OU["mu"], theta=ar.OU["theta"], sigma=sigma, device="cuda:0")
    block = torch.full((B + extra_rows, A), -77.25, dtype=torch.float64, device="cuda:0")
    block[:B].copy_(torch.from_numpy(start))
    ou.state = block[:B]
    return ou, block


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ar.CASES, ids=CASE_IDS)
def test_query_matches_host_replay(case, f16, record_property):
    torch = _torch()
    w, obs_np = ar.case_weights(case), ar.case_obs(case, f16)
    actor = _module(w)
    obs = torch.from_numpy(obs_np).cuda()
    B, A = case.B, case.A
    std = ar.device_std(ar.COV_VAR)
    plain, mean_q, noisy, noisy0 = [_device_actor(actor, case, 0) for _ in range(4)]
    ou, block = _ou(B, A, ar.OU["sigma"], ar.case_ou_start(case))
    ou0, block0 = _ou(B, A, 0.0, ar.case_ou_start(case))
    const = _logp_const(A, ar.COV_VAR)
    log, spread = [], 0.0
    try:
        for call in range(ar.N_CALLS):
            q = ar.case_query(case, w, obs_np, call)
            spread = max(spread, q.mean_f32_spread)
            action, log_prob, mean = _np(plain(obs, ar.COV_VAR))
            ar.check_mean(mean, q.mean, q.mean_f32_spread if case.name in ar.F32_SPREAD_CASES else None, f"mean: call {call}", log)
            ar.check_eps(action, mean, ar.COV_VAR, q.eps, f"eps: call {call}", log)
            ar.check_log_prob(log_prob, q.log_prob, f"log_prob: call {call}", log)
            # streams are separate: this call's eps is not the next call's
            assert ar.eps_differs(action, mean, ar.COV_VAR, ar.case_query(case, w, obs_np, call + 1).eps)
            # mean mode
            a_m, l_m, m_m = _np(mean_q(obs, ar.COV_VAR, action_mode="mean"))
            assert np.array_equal(a_m.view(np.uint32), m_m.view(np.uint32)), "mean mode: action != mean bit for bit"
            assert np.array_equal(m_m.view(np.uint32), mean.view(np.uint32)), "mean mode: another mean than the sampling query's"
            assert np.all(l_m == -const), (float(l_m[0]), -float(const))
            # OU term: sigma 0.05 and sigma 0
            for dev_actor, o, blk, sigma in ((noisy, ou, block, ar.OU["sigma"]), (noisy0, ou0, block0, 0.0)):
                s_before = o.state.cpu().numpy().copy()
                a_o, l_o, m_o = _np(dev_actor(obs, ar.COV_VAR, ou_noise=o))
                s_after = blk.cpu().numpy().copy()
                qo = ar.case_query(case, w, obs_np, call, ou_state=s_before, mu=ar.OU["mu"], theta=ar.OU["theta"], sigma=sigma)
                ar.check_ou_state(s_after[:B], qo.ou_state, sigma, f"ou_state: call {call} sigma {sigma}", log)
                assert np.all(s_after[B:] == -77.25), "OU rows past the batch were written"
                want = (action.astype(np.float64) + s_after[:B]).astype(np.float32)
                assert np.array_equal(a_o.view(np.uint32), want.view(np.uint32)), "action_ou != float32(float64(action) + state)"
                assert np.array_equal(m_o.view(np.uint32), mean.view(np.uint32)), "the OU term changed the mean"
                if A <= 16:   # one output tile: the order of log_prob's LDS atomics is fixed (test_gpu_action_noise.py)
                    assert np.array_equal(l_o.view(np.uint32), log_prob.view(np.uint32)), "the OU term changed log_prob"
                ar.check_log_prob(l_o, q.log_prob, f"log_prob: OU call {call}", log)
        assert plain.calls == mean_q.calls == noisy.calls == noisy0.calls == case.call_index + ar.N_CALLS
    finally:
        _report(record_property, log, f32_spread=spread)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ar.CASES, ids=CASE_IDS)
def test_zero_pattern_matches_host_replay(case, f16, record_property):
    """Layers 2 and 3 the identity, the output layer the first A rows of the identity: mean[e][m] = keep_scale^3 relu(layer 1)[e][m] where
    unit m survives all three masks, exactly zero elsewhere.  The set of zeros must be the reference's, element for element."""
    torch = _torch()
    w, obs_np = ar.case_weights(case, identity=True), ar.case_obs(case, f16)
    actor = _module(w)
    obs = torch.from_numpy(obs_np).cuda()
    da = _device_actor(actor, case, 0)
    log = []
    try:
        for call in range(ar.N_CALLS):
            q = ar.case_query(case, w, obs_np, call)
            zero, nonzero = ar.zero_pattern(w, obs_np, q.masks)
            _, _, mean = _np(da(obs, ar.COV_VAR))
            ar.check_zero_pattern(mean, zero, nonzero, f"zero pattern, call {call}")
            ar.check_mean(mean, q.mean, None, f"mean: identity call {call}", log)
    finally:
        _report(record_property, log)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_eps_without_recovery(f16, record_property):
    """Output weights and biases zero: the mean is exactly zero and action = std eps, so eps is read off without the rounding of
    action - mean.  Held to EPS_TOL alone; the largest deviation is the hardware's (v_log_f32, v_sqrt_f32, v_cos_f32 / v_sin_f32)."""
    torch = _torch()
    case = ar.CASES[0]
    w, obs_np = ar.case_weights(case), ar.case_obs(case, f16)
    w[6][:], w[7][:] = 0, 0
    actor = _module(w)
    obs = torch.from_numpy(obs_np).cuda()
    da = _device_actor(actor, case, 0)
    log = []
    try:
        for call in range(ar.N_CALLS):
            q = ar.case_query(case, w, obs_np, call)
            action, log_prob, mean = _np(da(obs, ar.COV_VAR))
            assert np.all(mean == 0)
            ar.check_eps(action, mean, ar.COV_VAR, q.eps, f"eps: direct call {call}", log, recovery=False)
            ar.check_log_prob(log_prob, q.log_prob, f"log_prob: call {call}", log)
    finally:
        _report(record_property, log)


@pytest.mark.parametrize("S,H", ar.UNSUPPORTED)
def test_unsupported_hidden_sizes(S, H):
    """One past the largest hidden size beside 1024 inputs, one past the widest hidden layer, and hidden 1024, which the dimension check
    lets through: AOG_ERR_UNSUPPORTED before any launch."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, make_actor

    B, A = 16, 16
    actor = make_actor(S, A, H, device="cuda:0")
    da = DeviceActor(actor, seed=1)
    net = da.net(B)
    obs = torch.zeros((B, S), dtype=torch.float16, device="cuda:0")
    out = torch.full((B, 2 * A + 1), 3.0, dtype=torch.float32, device="cuda:0")
    p = C.c_void_p
    rc = da.lib.aog_actor_act(C.byref(net), 0, p(obs.data_ptr()), 1, p(out.data_ptr()), p(out.data_ptr() + 4 * B * A), p(out.data_ptr() + 8 * B * A),
                              p(torch.cuda.current_stream().cuda_stream))
    assert rc == -4, (rc, da.lib.aog_last_error())   # AOG_ERR_UNSUPPORTED
    assert b"does not fit the LDS" in da.lib.aog_last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


TAIL_CASES = [ar.Case("tail_o2", 4, 150, 16, 70, 0.5, 0, 11, 0, 21, 100.0), ar.Case("tail_o32_separable", 1024, 150, 64, 20, 0.5, 0, 11, 0, 22, 100.0)]


@pytest.mark.parametrize("with_ou", [False, True], ids=["plain", "ou"])
@pytest.mark.parametrize("case", TAIL_CASES, ids=[c.name for c in TAIL_CASES])
def test_fused_tail_matches_host_replay(case, with_ou, record_property):
    """k_epilogue_act_prologue(_noise) directly: reset_with_policy + step_with_policy on quasi-static 64-pixel envs; the float16 observation
    each call returned and the call index it consumed go to the reference.  (That the prologue loads this action bit for bit like the
    unfused loop is test_gpu_step_act.py's assertion.)"""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.rollout import DeviceActor

    o, B, A, T = int(round(case.S ** 0.5)), case.B, case.A, 3
    env = BatchedAOEnv(B, "cuda:0", act_dim=A, obs_dim=o, num_pupil_pixels=64, timesteps_per_episode=T, screens=smooth_screens(B, 64, 2),
                       verbose=False)
    assert (env.obs_route == "separable") == (o == 32)
    w = ar.case_weights(case)
    actor = _module(w)
    da = DeviceActor(actor, seed=case.seed)
    ou, block = _ou(B, A, ar.OU["sigma"], ar.case_ou_start(case)) if with_ou else (None, None)
    kw = dict(ou_noise=ou) if with_ou else {}
    log, queries = [], 0
    try:
        for t in range(T):
            call = da.calls
            s_before = ou.state.cpu().numpy().copy() if with_ou else None
            if t == 0:
                (obs, _), pol = env.reset_with_policy(da, ar.COV_VAR, **kw)
            else:
                ret, pol = env.step_with_policy(da, ar.COV_VAR, **kw)
                obs = ret[0]
            assert pol is not None and da.calls == call + 1
            obs_np = obs.cpu().numpy().copy()
            assert obs_np.dtype == np.float16 and obs_np.shape == (B, case.S)
            action, log_prob, mean = _np(pol)
            s_after = block.cpu().numpy().copy() if with_ou else None
            q = ar.reference_query(w, obs_np, case.p, ar.COV_VAR, case.seed, call, 0, ou_state=s_before, **(ar.OU if with_ou else {}))
            ar.check_mean(mean, q.mean, None, f"mean: query {t}", log)
            ar.check_eps(action, mean, ar.COV_VAR, q.eps, f"eps: query {t}", log, ou_state_dev=s_after[:B] if with_ou else None)
            ar.check_log_prob(log_prob, q.log_prob, f"log_prob: query {t}", log)
            if with_ou:
                ar.check_ou_state(s_after[:B], q.ou_state, ar.OU["sigma"], f"ou_state: query {t}", log)
                assert np.all(s_after[B:] == -77.25), "OU rows past the batch were written"
            queries += 1
        ret, pol = env.step_with_policy(da, ar.COV_VAR, **kw)   # the episode's last step queries nothing
        assert pol is None and queries == T and da.calls == T
        assert env.device_status() == 0
    finally:
        _report(record_property, log)
        env.close()
