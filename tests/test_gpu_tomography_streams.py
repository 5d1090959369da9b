"""Every entry point of ``include/aogym_tomography.h`` that takes a stream, run on a caller's side stream behind a delayed producer
(``stream_harness``, through ``test_gpu_streams._both``) and held bit for bit to a twin that makes the same calls on the default stream.
``test_tomography_stream_coverage_cpu.py`` checks that the tables below place every such entry point."""
import numpy as np
import pytest

from test_gpu_streams import _acts, _both, _env, _torch, cycles_per_ms  # noqa: F401  (cycles_per_ms: the module's calibration fixture)

pytestmark = pytest.mark.gpu

# entry point (include/aogym_tomography.h, every one with a `void* stream`) -> the test here that drives it through Python
COVERED = {
    "aog_wavefront_project": "test_projection", "aog_tomo_upload": "test_tomograph", "aog_tomo_update": "test_tomograph",
    "aog_tomo_reset": "test_tomograph", "aog_tomo_get_state": "test_tomograph", "aog_tomo_set_state": "test_tomograph",
}
NOT_DRIVEN = {}


def test_projection(cycles_per_ms):  # noqa: F811
    torch = _torch()
    from adaptive_optics_gym_amd import tomography as tm

    B, N, A = 5, 32, 6
    screens = np.random.RandomState(1).randn(B, N, N) * 2 * np.pi * 1e-7

    def make():
        env = _env(B, N, screens=screens, timesteps_per_episode=5)
        tm.upload_wavefront_shapes(env, np.random.RandomState(2).randn(40, int(env.tables.n_ap)))
        return env

    def script(env, r):
        r.call("reset", lambda: env.reset()[0])
        mean = torch.zeros((B,), dtype=torch.float64, device="cuda")
        r.call("project", lambda: (tm.wavefront_project(env, mean=mean), mean), weight=2)
        for t in range(2):
            a = r.input(_acts(B, A, t, 0.3))
            r.call(f"step{t} + project", lambda: (env.step(a), tm.wavefront_project(env)), weight=3)

    _both(cycles_per_ms, make, script)


def test_tomograph(cycles_per_ms):  # noqa: F811
    from adaptive_optics_gym_amd.device_handle import ptr
    from adaptive_optics_gym_amd.tomography import DeviceTomograph

    B, K, widths = 5, 15, (15, 6)
    rng = np.random.RandomState(3)
    R = [rng.randn(K, J) for J in widths]
    S = [[rng.randn(B, J) * 1e-7 for J in widths] for _ in range(5)]

    def make():
        return DeviceTomograph(B, K, widths)

    def script(h, r):
        # the matrices, uploaded on the caller's stream (the inputs stay alive: no wait): the update behind them reads them
        ms, s = [r.input(m) for m in R], [r.input(x) for x in S[0]]
        r.call("uploads + update0", lambda: (h._call("upload", 0, ptr(ms[0]), h._stream()), h._call("upload", 1, ptr(ms[1]), h._stream()),
                                             h.update(s, 0.5, 0.99, 1e-7))[2], weight=3)
        s = [r.input(x) for x in S[1]]
        r.call("update1", lambda: h.update(s, 0.5, 0.99, 1e-7))
        s, m = [r.input(x) for x in S[2]], r.input(np.array([True, False, True, True, False]))
        r.call("masked update", lambda: h.update(s, 0.5, 0.99, 0.0, m))
        m = r.input(np.array([False, True, False, False, True]))
        s = [r.input(x) for x in S[3]]
        r.call("masked reset + update", lambda: (h.reset(m), h.update(s, 0.5))[1], weight=2)
        blob = r.call("get_state", lambda: h.get_state())
        s, b = [r.input(x) for x in S[4]], r.input(blob)
        r.call("update + reset + set_state", lambda: (h.update(s, 0.5), h.reset(), h.set_state(b))[0], blocking="set_state", weight=3)
        s = [r.input(x) for x in S[0]]
        r.call("update after set_state", lambda: (h.update(s, 0.5), h.get_state()), weight=2)

    _both(cycles_per_ms, make, script)
