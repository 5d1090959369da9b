"""The off-step instruments of one handle (wavefront fit, output gradient, science camera, pyramid sensor and its gradient) share one
actuator scratch: a call must get nothing from the call before it.  Every result is compared bit for bit between a handle that makes the
calls in one order, a twin that makes them in the reverse order and fresh twins that make one call each.

Calibration: on the parent commit, where every instrument had a scratch of its own, all of these comparisons hold exactly for both
atmospheres (MI355X), so every one is held to ``torch.equal`` here."""
import numpy as np
import pytest

from helpers import actions_for

pytestmark = pytest.mark.gpu

# one full env tile and a ragged one; the smallest science window and the smallest pyramid the host tables accept at N = 32
B, N, A, O = 37, 32, 6, 8
KW = dict(act_type="num_actuators", act_dim=A, obs_dim=O, obs_gradient=True, num_pupil_pixels=N, timesteps_per_episode=5, seed=29,
          science_window=2, pyramid=dict(samples=16, pixels=16, n_mod=2), verbose=False)
ORDER = ("truth", "gradient", "science", "slopes", "pyramid_gradient", "truth_again")
_TABLES = {}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _env(atm):
    """A twin: same seed, same tables, one reset and two steps with non-zero actions."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from adaptive_optics_gym_amd.optics_host import build_tables, obs_route_for
    from adaptive_optics_gym_amd.params import OpticalParams

    if not _TABLES:   # the host precompute once; every handle shares it
        _TABLES[0] = build_tables(OpticalParams(num_pupil_pixels=N), "num_actuators", A, O, obs_route=obs_route_for("fast", O))
    env = BatchedAOEnv(B, "cuda:0", tables=_TABLES[0], **KW, **atm)
    assert env.obs_route == "separable" and env.obs_gradient
    env.reset()
    for t in range(2):
        env.step(torch.from_numpy(actions_for(B, A, 40 + t)).cuda())
    return env


def _inputs(env):
    torch = _torch()
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(a).cuda()
    return dict(g_obs=dev(rng.standard_normal((B, O * O))), g_power=dev(rng.standard_normal(B)), g_strehl=dev(rng.standard_normal(B)),
                g_slopes=dev(rng.standard_normal((B, 2 * env._pyramid.n_valid))), X=dev(5e-8 * rng.standard_normal((B, A))))


def _call(env, name, x):
    """One instrument call; its results as a tuple of tensors."""
    if name in ("truth", "truth_again"):
        out = env.wavefront_truth()
        return tuple(out[k] for k in ("rms", "fit_rms", "coef", "ideal_actuators"))
    if name == "gradient":
        return env.output_gradient(x["g_obs"], x["g_power"], x["g_strehl"], with_values=True)
    if name == "science":
        env.science_integrate()
        out = env.science_exposure()
        return tuple(out[k] for k in ("psf", "strehl", "encircled_energy", "frames"))
    if name == "slopes":
        return (env.pyramid_slopes(),)
    return env.pyramid_gradient(g_slopes=x["g_slopes"], actuators=x["X"], with_values=True)   # (X is not the mirror's actuators)


def _run(atm, names):
    env = _env(atm)
    try:
        x = _inputs(env)
        assert not _torch().equal(x["X"], env.get_actuators())
        return {n: tuple(t.clone() for t in _call(env, n, x)) for n in names}
    finally:
        env.close()


@pytest.mark.parametrize("atm", [dict(atm_type="quasi_static"), dict(atm_type="dynamic", atm_vel=20.0)], ids=["quasi_static", "dynamic"])
def test_no_call_reads_what_another_left_in_the_shared_scratch(atm):
    torch = _torch()
    forward, reverse = _run(atm, ORDER), _run(atm, ORDER[::-1])
    fresh = {}
    for n in ORDER[:-1]:
        fresh.update(_run(atm, (n,)))
    fresh["truth_again"] = fresh["truth"]
    for n in ORDER:
        assert len(forward[n]) == len(reverse[n]) == len(fresh[n])
        for i, (f, r, s) in enumerate(zip(forward[n], reverse[n], fresh[n])):
            assert bool(torch.isfinite(f.double()).all()), (n, i)
            assert torch.equal(f, r), (n, i, "forward order vs reverse order")
            assert torch.equal(f, s), (n, i, "in sequence vs alone on a fresh handle")
    # the actuators=X of the pyramid gradient did not survive into the wavefront fit after it
    for i, (first, again) in enumerate(zip(forward["truth"], forward["truth_again"])):
        assert torch.equal(first, again), i
    assert float(forward["pyramid_gradient"][0].abs().max()) > 0 and float(forward["gradient"][0].abs().max()) > 0
