"""Every entry point of ``include/aogym_servo.h`` that takes a stream, run on a caller's side stream behind a delayed producer
(``stream_harness``, through ``test_gpu_streams._both``) and held bit for bit to a twin that makes the same calls on the default stream.
``test_servo_stream_coverage_cpu.py`` checks that the tables below place every such entry point."""
import numpy as np
import pytest

from test_gpu_streams import _acts, _both, _env, _torch, cycles_per_ms  # noqa: F401  (cycles_per_ms: the module's calibration fixture)

pytestmark = pytest.mark.gpu

# entry point (include/aogym_servo.h, every one with a `void* stream`) -> the test here that drives it through Python
COVERED = {
    "aog_servo_reset": "test_servo", "aog_servo_apply": "test_servo", "aog_servo_get_state": "test_servo", "aog_servo_set_state": "test_servo",
}
NOT_DRIVEN = {}

SERVO = dict(latency=[0.0, 1.0, 1.5, 2.0, 0.5], response=[1.0, 0.5, 0.1, 1.0, 0.5], stroke=[np.inf, 0.8, np.inf, 0.8, np.inf], stuck={1: 0.25})


def test_servo(cycles_per_ms):  # noqa: F811
    torch = _torch()
    from adaptive_optics_gym_amd import MirrorServo

    B, N, A = 5, 32, 6

    def make():
        env = _env(B, N, screens=np.zeros((B, N, N)))
        return env, MirrorServo(env, **SERVO)

    def script(h, r):
        _, servo = h
        for t in range(3):
            a = r.input(_acts(B, A, t))
            r.call(f"apply{t}", lambda: servo.apply(a))
        a, m = r.input(_acts(B, A, 3)), r.input(np.array([True, False, True, True, False]))
        out = torch.full((B, A), 7.0, device="cuda")
        r.call("masked apply", lambda: servo.apply(a, m, out=out))
        a, m = r.input(_acts(B, A, 4)), r.input(np.array([False, True, False, False, True]))
        r.call("masked reset + apply", lambda: (servo.reset(m), servo.apply(a))[1], weight=2)
        blob = r.call("get_state", lambda: servo.get_state())
        a, b = r.input(_acts(B, A, 5)), r.input(blob)
        r.call("apply + reset + set_state", lambda: (servo.apply(a), servo.reset(), servo.set_state(b))[0], blocking="set_state", weight=3)
        a = r.input(_acts(B, A, 6))
        r.call("apply after set_state", lambda: (servo.apply(a), servo.get_state()), weight=2)

    _both(cycles_per_ms, make, script)


def test_env_with_a_servo(cycles_per_ms):  # noqa: F811
    B, N, A = 5, 32, 6
    mask = np.array([True, False, True, True, False])

    def make():
        return _env(B, N, screens=np.zeros((B, N, N)), timesteps_per_episode=5, servo=SERVO)

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        for t in range(3):
            a = r.input(_acts(B, A, t, 0.3))
            r.call(f"step{t}", lambda: env.step(a), weight=2)   # (the servo's launch, then the step)
        m = r.input(mask)
        r.call("masked reset", lambda: env.reset(m)[0], weight=2)
        a = r.input(_acts(B, A, 3, 0.3))
        r.call("step after the masked reset", lambda: env.step(a), weight=2)
        state = r.call("get_state", lambda: env.get_state(), blocking="get_state")
        a = r.input(_acts(B, A, 4, 0.3))
        r.call("step after get_state", lambda: env.step(a), weight=2)
        a = r.input(_acts(B, A, 4, 0.3))
        r.call("set_state + step", lambda: (env.set_state(state), env.step(a))[1], blocking="set_state", weight=3)

    _both(cycles_per_ms, make, script)
