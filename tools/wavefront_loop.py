"""Timing of aog_wavefront_truth (BatchedAOEnv.wavefront_truth) at config-2 shape beside a step of the same handle, and (--rollout) of
rollout(policy='ideal') against policy='shack' at config 4's shape.  Under rocprofv3 --kernel-trace --stats the kernel table shows
k_wavefront_fit / k_wavefront_finish next to k_fused_tab of the same run (profiles/wavefront_truth.md).

    python tools/wavefront_loop.py            # the call and a step, wall time per call after a warm-up under load
    python tools/wavefront_loop.py --rollout  # episodes of the two controllers at B = 1024, N = 256, A = 64, dynamic v = 10 m/s"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adaptive_optics_gym_amd import BatchedAOEnv
from adaptive_optics_gym_amd.rollout import rollout

B, N, A = 1024, 256, 64


def timed(fn, n, warm_s=0.5):
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < warm_s:   # the device needs a few hundred ms of load to reach its clocks
        fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


if "--rollout" in sys.argv:
    env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=10, atm_fried=0.15, act_dim=A, obs_dim=2, num_pupil_pixels=N, seed=3,
                       screen_oversampling=4, timesteps_per_episode=20, SH_operation=True, verbose=False)
    for pol in ("ideal", "shack"):
        rollout(env, None, episodes=1, policy=pol)
        torch.cuda.synchronize()
        t0, n_ep = time.perf_counter(), 3
        out = rollout(env, None, episodes=n_ep, policy=pol)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / (n_ep * 20)
        print(f"rollout(policy={pol!r}) B={B} N={N} A={A} dynamic: {dt * 1e3:.3f} ms per step ({B / dt:.0f} env-steps/s), avg_ep_rew {out['avg_ep_rew']:.4f}")
else:
    env = BatchedAOEnv(B, "cuda:0", act_dim=A, obs_dim=2, num_pupil_pixels=N, seed=3, screen_oversampling=4, timesteps_per_episode=10 ** 6,
                       verbose=False)
    env.reset()
    a = torch.randn(B, A, device="cuda")
    env.step(a)
    out = env.wavefront_truth()
    dt = timed(lambda: env.wavefront_truth(out=out), 20)
    n_ap, n_pt = env.tables.n_ap, env.info.n_ap_padded // 32
    mb = (B * n_pt * 32 * 4 + 2 * n_pt * 32 * A * 4) / 1e6   # the screens once, the two mode layouts once (f16 hi + lo each)
    print(f"aog_wavefront_truth B={B} N={N} A={A}: {dt * 1e6:.1f} us per call; {mb:.0f} MB read once = {mb / 1e6 / dt:.2f} TB/s")
    dt_s = timed(lambda: env.step(a), 20)
    print(f"step of the same handle: {dt_s * 1e6:.1f} us per call")
