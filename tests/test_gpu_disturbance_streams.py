"""Every entry point of ``include/aogym_disturbance.h`` that takes a stream, run on a caller's side stream behind a delayed producer
(``stream_harness``, through ``test_gpu_streams._both``) and held bit for bit to a twin that makes the same calls on the default stream.
``test_disturbance_stream_coverage_cpu.py`` checks that the tables below place every such entry point."""
import numpy as np
import pytest

from test_gpu_streams import _acts, _both, _env, _torch, cycles_per_ms  # noqa: F401  (cycles_per_ms: the module's calibration fixture)

pytestmark = pytest.mark.gpu

# entry point (include/aogym_disturbance.h, every one with a `void* stream`) -> the test here that drives it through Python
COVERED = {
    "aog_disturbance_reset": "test_generator", "aog_disturbance_advance": "test_generator", "aog_disturbance_coefficients": "test_generator",
    "aog_disturbance_get_state": "test_generator", "aog_disturbance_set_state": "test_generator",
    "aog_install_layer_sum_disturbed": "test_layered_with_a_disturbance",
}
NOT_DRIVEN = {}

VIB = [dict(term=0, frequency=60.0, damping=0.05, rms=4e-8), dict(term=1, frequency=[20.0, 30.0, 40.0, 50.0, 60.0], damping=0.1, rms=2e-8)]


def test_generator(cycles_per_ms):  # noqa: F811
    torch = _torch()
    from adaptive_optics_gym_amd import ModalDisturbance

    B, N, K = 5, 32, 3

    def make():
        env = _env(B, N, screens=np.zeros((B, N, N)))
        return env, ModalDisturbance(env, ["tip", "tilt", "focus"], vibrations=VIB, static=[0.0, 1e-8, -3e-8], seed=7)

    def script(h, r):
        _, gen = h
        r.call("advance", lambda: gen.advance())
        m = r.input(np.array([True, False, True, True, False]))
        noise = torch.zeros((B, K), dtype=torch.float64, device="cuda")
        r.call("masked advance", lambda: (gen.advance(m, noise_out=noise), noise))
        r.call("coefficients", lambda: gen.coefficients())
        m = r.input(np.array([False, True, False, False, True]))
        start = torch.zeros((B, K, 2), dtype=torch.float64, device="cuda")
        r.call("masked reset + advance", lambda: (gen.reset(m, noise_out=start), gen.advance(), start)[1:], weight=2)
        blob = r.call("get_state", lambda: gen.get_state())
        b = r.input(blob)
        r.call("reset + set_state + advance", lambda: (gen.reset(), gen.set_state(b), gen.advance(), gen.get_state())[2:], blocking="set_state", weight=3)

    _both(cycles_per_ms, make, script)


def test_layered_with_a_disturbance(cycles_per_ms):  # noqa: F811
    from adaptive_optics_gym_amd import LayeredAOEnv

    B, A, N = 5, 6, 32
    layers = [{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}]

    def make():
        return LayeredAOEnv(B, "cuda:0", atm_layers=layers, atm_fried=0.15, seed=11, act_type="zernike", act_dim=A, obs_dim=2, rew_type="strehl_ratio",
                            timesteps_per_episode=5, num_pupil_pixels=N, verbose=False,
                            disturbance=dict(shapes=["tip", "focus"], vibrations=VIB[:1], static=[0.0, 3e-8]))

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        for t in range(3):
            a = r.input(_acts(B, A, t))
            # (every layer evolves, the generator advances and ticks, the sum is installed, then the step)
            r.call(f"step{t}", lambda: (env.step(a), env.disturbance.coeff), weight=len(layers) + 4)
        state = r.call("get_state", lambda: env.get_state(), blocking="get_state")
        a = r.input(_acts(B, A, 3))
        r.call("step after get_state", lambda: env.step(a), weight=len(layers) + 4)
        a = r.input(_acts(B, A, 3))
        r.call("set_state + step", lambda: (env.set_state(state), env.step(a), env.disturbance.coeff)[1:], blocking="set_state")

    _both(cycles_per_ms, make, script)
