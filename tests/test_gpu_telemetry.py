"""The modal telemetry on the device (aog_telemetry_*, csrc/k_telemetry.h) against its numpy restatement (tests/telemetry_reference.py):
the ring, Welch's PSD and the cost J inside FACTOR x the restatement's own float64-versus-longdouble envelope, the argmin exactly, and
the bit-for-bit properties (split batch, mask, checkpoint); then ModalIntegrator and rollout(policy="modal").

FACTOR: the device sums in another order than the restatement (a radix-2 FFT against a dense DFT), so its distance from the float64
restatement is of the size of that restatement's own rounding, the envelope.  Measured ratios are in profiles/telemetry.md."""
import numpy as np
import pytest

import telemetry_reference as ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
GAP = 1e-9
# (B, A, T, S, delay, samples pushed): one env tile and more than one (35: no multiple of 32); A below a wave, a wave, two mode blocks; the
# ring wrapped by 17 rows so that a segment straddles the seam; S = T (one segment, the whole ring); the headline segment at T = 512
CASES = [(3, 5, 64, 32, 1, 81), (35, 64, 64, 64, 2, 81), (35, 128, 64, 32, 1, 81), (3, 128, 64, 64, 2, 64), (3, 64, 512, 128, 1, 529)]
IDS = [f"B{b}_A{a}_T{t}_S{s}_d{d}_n{n}" for b, a, t, s, d, n in CASES]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _tel(B, A, T):
    from adaptive_optics_gym_amd.telemetry import ModalTelemetry

    return ModalTelemetry(B, A, length=T, device="cuda:0")


def _grid(d):
    from adaptive_optics_gym_amd.telemetry import default_grid

    return default_grid(d)


def _series(seed, n, B, A):
    """[n, B, A]: AR(1) modes whose size falls by 1e6 from the first mode to the last, each around a mean 1e4 times its fluctuation."""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** (-6.0 * np.arange(A) / max(A - 1, 1))
    pole = rng.uniform(0.5, 0.999, size=(B, A))
    x = np.zeros((n, B, A))
    e = rng.randn(n, B, A)
    for t in range(1, n):
        x[t] = pole * x[t - 1] + e[t]
    x = x + rng.uniform(0.05, 1.0, size=(B, A)) * rng.randn(n, B, A)
    return (x + 1e4 * np.where(rng.rand(B, A) < 0.5, -1.0, 1.0)) * scale


_CASE_CACHE = {}


def _case(B, A, T, S, d, n):
    """The inputs of a case and their reference results, computed once: the seed is the first whose best and second-best J differ by more
    than GAP (relative) for every (env, mode) in the float64 reference."""
    key = (B, A, T, S, d, n)
    if key in _CASE_CACHE:
        return _CASE_CACHE[key]
    grid = _grid(d)
    for seed in range(100, 120):
        x = _series(seed, n, B, A)
        ring = ref.RingReference(B, A, T)
        for y in x:
            ring.push(y)
        res = {name: [ref.optimise(ring.series(b), S, d, grid, dt) for b in range(B)] for name, dt in (("f64", np.float64), ("ld", np.longdouble))}
        J = np.stack([r[2] for r in res["f64"]])
        two = np.sort(J, axis=-1)[..., :2]
        if np.all(two[..., 1] - two[..., 0] > GAP * two[..., 1]):
            break
    else:
        raise AssertionError("no seed separates the best two candidates")
    out = {"x": x, "grid": grid, "ring": ring}
    for name in ("f64", "ld"):
        out[name] = {"gain": np.stack([r[0] for r in res[name]]), "cost": np.stack([r[1] for r in res[name]]), "J": np.stack([r[2] for r in res[name]]),
                     "phi": np.stack([r[3] for r in res[name]]), "nseg": np.array([r[4] for r in res[name]])}
    for v in out["f64"].values():
        v.setflags(write=False)
    _CASE_CACHE[key] = out
    return out


def _push_all(torch, tel, x, masks=None):
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for t in range(xd.shape[0]):
        tel.push(xd[t], None if masks is None else masks[t])


def _bound(label, got, f64, ld):
    """got within FACTOR x the envelope of the case, per row as a fraction of the row's largest value."""
    env = float(ref.row_error(f64, ld).max())
    err = float(ref.row_error(got, f64).max())
    print(f"{label}: envelope {env:.3e}  device {err:.3e}  ({err / env if env else float('inf'):.2f} x)")
    assert 0 < env < 1e-9, "the inputs are ill-conditioned: change them, do not widen the factor"
    assert err <= FACTOR * env


# ---- 1. the ring -------------------------------------------------------------------------------------------------------------------------
def test_ring_counts_wraps_skips_masks_and_resets():
    torch = _torch()
    B, A, T, S = 3, 5, 64, 32
    x = _series(5, T + 17, B, A)
    tel, ring = _tel(B, A, T), ref.RingReference(B, A, T)
    grid = _grid(1)

    def same_state():
        st = tel.unpack()
        return (np.array_equal(st["hist"].cpu().numpy(), ring.hist) and np.array_equal(st["count"].cpu().numpy(), ring.count)
                and np.array_equal(st["skipped"].cpu().numpy(), ring.skipped))

    _push_all(torch, tel, x[:S - 1])
    for y in x[:S - 1]:
        ring.push(y)
    freq, psd, seg = tel.psd(S)
    gain, cost, cost_all = tel.optimise_gains(1, grid, S, with_costs=True)
    assert tuple(psd.shape) == (B, A, S // 2 + 1) and bool(torch.isnan(psd).all()) and not bool(seg.any()) and seg.dtype == torch.int32
    assert bool(torch.isnan(gain).all()) and bool(torch.isnan(cost).all()) and bool(torch.isnan(cost_all).all())
    assert np.array_equal(freq.cpu().numpy(), np.arange(S // 2 + 1) / S)
    _push_all(torch, tel, x[S - 1:S])
    ring.push(x[S - 1])
    _, psd, seg = tel.psd(S)
    assert seg.tolist() == [1, 1, 1] and same_state()
    want = [ref.welch_psd(ring.series(b), S, dt)[0] for dt in (np.float64, np.longdouble) for b in range(B)]
    _bound("count = S", psd.cpu().numpy(), np.stack(want[:B]), np.stack(want[B:]))
    # masked pushes leave env 1 alone; a row with a NaN (env 2) or an infinity (env 0) is skipped and counted
    for t in range(S, T + 17):
        y = x[t].copy()
        mask = [True, t % 3 != 0, True]
        if t == S + 4:
            y[2, A - 1] = np.nan
        if t == S + 9:
            y[0, 0] = -np.inf
        tel.push(torch.from_numpy(y).cuda(), torch.tensor(mask))
        ring.push(y, mask)
    assert same_state() and list(ring.skipped) == [1, 0, 1] and ring.count[0] == T + 16 > T
    _, psd, seg = tel.psd(S)
    want = [ref.welch_psd(ring.series(b), S, dt) for dt in (np.float64, np.longdouble) for b in range(B)]
    assert seg.tolist() == [w[1] for w in want[:B]] == [3, 3, 3]
    _bound("wrapped ring", psd.cpu().numpy(), np.stack([w[0] for w in want[:B]]), np.stack([w[0] for w in want[B:]]))
    tel.reset(torch.tensor([False, True, False]))
    ring.reset([False, True, False])
    assert same_state() and ring.count[1] == 0
    _, psd, seg = tel.psd(S)
    assert seg.tolist() == [3, 0, 3] and bool(torch.isnan(psd[1]).all()) and bool(torch.isfinite(psd[0]).all())
    tel.close()


# ---- 2. PSD, cost and argmin against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,T,S,d,n", CASES, ids=IDS)
def test_psd_cost_and_gains_against_the_reference(B, A, T, S, d, n):
    torch = _torch()
    c = _case(B, A, T, S, d, n)
    tel = _tel(B, A, T)
    _push_all(torch, tel, c["x"])
    _, psd, seg = tel.psd(S)
    gain, cost, cost_all = tel.optimise_gains(d, c["grid"], S, with_costs=True)
    f64, ld = c["f64"], c["ld"]
    assert np.array_equal(seg.cpu().numpy(), f64["nseg"]) and f64["nseg"].min() >= 1
    assert np.array_equal(tel.unpack()["hist"].cpu().numpy(), c["ring"].hist)
    label = f"B={B} A={A} T={T} S={S} d={d}"
    _bound(label + " Phi", psd.cpu().numpy(), f64["phi"], ld["phi"])
    _bound(label + " J", cost_all.cpu().numpy(), f64["J"], ld["J"])
    assert np.array_equal(gain.cpu().numpy(), f64["gain"])          # the argmin, for every (env, mode)
    assert torch.equal(cost, cost_all.min(dim=-1).values)
    # without the table of every cost the call returns the same bits
    gain2, cost2 = tel.optimise_gains(d, c["grid"], S)
    assert torch.equal(gain2, gain) and torch.equal(cost2, cost)
    tel.close()


def test_a_tie_goes_to_the_first_candidate_in_grid_order():
    torch = _torch()
    B, A, T, S = 2, 5, 64, 32
    tel = _tel(B, A, T)
    y = torch.ones((B, A), dtype=torch.float64, device="cuda") * torch.arange(1, A + 1, dtype=torch.float64, device="cuda")
    for _ in range(S + 3):
        tel.push(y)          # constant rows: every deviation from the segment mean is exactly 0, so Phi = 0 and J(g) = 0 for every g
    _, psd, _ = tel.psd(S)
    assert not bool(psd.any())
    for d, grid in ((1, np.array([0.3, 0.5, 0.7, 0.9, 1.1, 1.3, 1.5])), (2, _grid(2))):
        gain, cost, cost_all = tel.optimise_gains(d, grid, S, with_costs=True)
        assert not bool(cost_all.any()) and not bool(cost.any())
        assert bool((gain == grid[0]).all())
    tel.close()


# ---- 3. bit for bit ----------------------------------------------------------------------------------------------------------------------------
def _results(tel, S, d, grid, mask=None):
    _, psd, seg = tel.psd(S, mask=mask)
    gain, cost, cost_all = tel.optimise_gains(d, grid, S, with_costs=True, mask=mask)
    return psd, seg, gain, cost, cost_all


@pytest.mark.parametrize("B,A,T,S,d,n", [CASES[0], CASES[1], CASES[4]], ids=[IDS[0], IDS[1], IDS[4]])
def test_split_batch_mask_and_checkpoint_reproduce_the_bits(B, A, T, S, d, n):
    torch = _torch()
    c = _case(B, A, T, S, d, n)
    x, grid = c["x"], c["grid"]
    whole = _tel(B, A, T)
    _push_all(torch, whole, x)
    want = _results(whole, S, d, grid)
    # two handles of ceil(B / 2) and floor(B / 2)
    h = (B + 1) // 2
    for lo, hi in ((0, h), (h, B)):
        part = _tel(hi - lo, A, T)
        _push_all(torch, part, x[:, lo:hi])
        for got, w in zip(_results(part, S, d, grid), want):
            assert torch.equal(got, w[lo:hi])
        assert torch.equal(part.get_state(), whole.get_state().view(B, -1)[lo:hi].reshape(-1))
        part.close()
    # masked calls give the selected envs the same bits and leave the others' rows alone
    mask = torch.arange(B) % 3 != 1
    for got, w in zip(_results(whole, S, d, grid, mask=mask), want):
        assert torch.equal(got[mask.cuda()], w[mask.cuda()])
        rest = got[~mask.cuda()]
        assert bool(torch.isnan(rest).all()) if rest.dtype == torch.float64 else not bool(rest.any())
    # a checkpoint taken part-way resumes in a fresh handle
    k = n - 9
    a, b = _tel(B, A, T), _tel(B, A, T)
    _push_all(torch, a, x[:k])
    b.load_state_dict(a.state_dict())
    _push_all(torch, b, x[k:])
    for got, w in zip(_results(b, S, d, grid), want):
        assert torch.equal(got, w)
    assert torch.equal(b.get_state(), whole.get_state())
    for t in (whole, a, b):
        t.close()


# ---- 4. the integrator and the rollout -----------------------------------------------------------------------------------------------------------
ENV_KW = dict(atm_type="dynamic", atm_vel=20.0, SH_operation=True, act_dim=16, obs_dim=2, num_pupil_pixels=32, rew_type="strehl_ratio", seed=17,
              verbose=False, pyramid=dict(samples=16, pixels=16, n_mod=4, r_mod=2.0))


def _record(ctrl):
    ys, inner = [], ctrl.update

    def update(y, mask=None):
        ys.append(y.clone())
        return inner(y, mask)

    ctrl.update = update
    return ys


def test_modal_integrator_and_rollout():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, ModalIntegrator, ModalTelemetry
    from adaptive_optics_gym_amd.rollout import rollout

    B, A, T = 8, 16, 40
    env = BatchedAOEnv(B, "cuda:0", timesteps_per_episode=T, **ENV_KW)
    ctrl = ModalIntegrator(env, measurement="truth", gain=0.4, telemetry=ModalTelemetry(B, A, length=64, device=env.device))
    ys = _record(ctrl)
    out = rollout(env, None, episodes=1, policy="modal", controller=ctrl)
    assert len(ys) == T and tuple(out["act"].shape) == (T, B, A) and bool((out["log_prob"] == 1).all())
    assert bool(torch.isfinite(out["ep_returns"]).all()) and bool(torch.isfinite(out["rew"]).all())
    a = torch.zeros((B, A), dtype=torch.float64, device="cuda")
    for t, y in enumerate(ys):                       # a plain integrator over the same measurements
        a = a + 0.4 * (y - a)
        assert torch.equal(out["act"][t], a.float()), t
    assert torch.equal(ctrl.command, a)
    st = ctrl.telemetry.unpack()
    assert st["count"].tolist() == [T] * B and torch.equal(st["hist"][:, :T], torch.stack(ys, dim=1))
    cost = ctrl.retune(segment=32)
    gain, cost2 = ctrl.telemetry.optimise_gains(1, None, 32)
    assert torch.equal(ctrl.gains, gain) and torch.equal(cost, cost2) and bool(torch.isfinite(gain).all())
    assert float(gain.min()) > 0
    # the pyramid's measurement feeds the same integrator
    pyr = ModalIntegrator(env, measurement="pyramid", gain=0.3, telemetry=ModalTelemetry(B, A, length=64, device=env.device))
    out = rollout(env, None, episodes=1, policy="modal", controller=pyr)
    assert bool(torch.isfinite(out["ep_returns"]).all()) and pyr.telemetry.unpack()["count"].tolist() == [T] * B
    ctrl.close()
    pyr.close()
    env.close()


def test_the_other_policies_keep_their_bits():
    """rollout(policy="pyramid") and rollout(policy="predictive") against the loops they have always been, on twin envs in the same run."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.predictor import PredictiveController
    from adaptive_optics_gym_amd.rollout import rollout

    B, T = 8, 6
    one, two = (BatchedAOEnv(B, "cuda:0", timesteps_per_episode=T, **ENV_KW) for _ in range(2))
    ctrls = [PredictiveController(e, order=2, measurement="truth") for e in (one, two)]
    for policy, kw, act_of in (("pyramid", {}, lambda: two.PYR_step()[0]), ("predictive", dict(predictor=ctrls[0]), ctrls[1].action)):
        out = rollout(one, None, episodes=1, policy=policy, **kw)
        obs, _ = two.reset()
        assert torch.equal(out["obs"][0], obs)
        for t in range(T):
            act = act_of().float()
            obs, rew, done, _, _ = two.step(act)
            assert torch.equal(out["act"][t], act) and torch.equal(out["rew"][t], rew) and torch.equal(out["next_obs"][t], obs), (policy, t)
    for c in ctrls:
        c.close()
    one.close()
    two.close()
