"""Times of aog_wavefront_project against wavefront_truth() and of aog_tomo_update, at the shape of profiles/tomography.md:
``python tools/tomography_time.py [num_envs] [N] [A]``.  HIP events around 200 calls, the median of 9 rounds after 3 warm-up rounds, the compared calls interleaved."""
import sys

import numpy as np
import torch

from adaptive_optics_gym_amd import BatchedAOEnv
from adaptive_optics_gym_amd import tomography as tm


def timed(fns, calls=200, rounds=9, warm=3):
    """{name: (median, min, max) us per call}: rounds of `calls` back-to-back calls between two HIP events (20 .. 70 ms of work per round),
    the versions taking turns inside every round so that clock and temperature drift falls on all of them alike."""
    out = {k: [] for k in fns}
    for r in range(warm + rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            if r >= warm:
                out[k].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in out.items()}


def main():
    B, N, A = (int(x) for x in (sys.argv[1:4] + ["1024", "256", "64"][len(sys.argv) - 1:]))
    env = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_fried=0.1, act_type="num_actuators", act_dim=A, obs_dim=2, num_pupil_pixels=N, seed=1,
                       verbose=False)
    env.reset()
    env.wavefront_truth()
    print(f"B={B} N={N} A={A} n_ap={int(env.tables.n_ap)}")
    rng = np.random.RandomState(0)
    for K in (64, 145):
        tm.upload_wavefront_shapes(env, rng.randn(K, int(env.tables.n_ap)))
        out = torch.empty((B, K), dtype=torch.float64, device="cuda")
        res = timed({"wavefront_truth": env.wavefront_truth, f"wavefront_project K={K}": lambda: tm.wavefront_project(env, out=out)})
        for k, v in res.items():
            print(f"{k}  us (median, min, max): %.1f %.1f %.1f" % v)
        print(f"ratio K={K}: %.3f" % (res[f"wavefront_project K={K}"][0] / res["wavefront_truth"][0]))
    K = 145
    tomo = tm.DeviceTomograph(B, K, (K, K))
    for g in range(2):
        tomo.upload(g, rng.randn(K, K))
    s = [torch.from_numpy(rng.randn(B, K) * 1e-7).cuda() for _ in range(2)]
    u = torch.empty((B, K), dtype=torch.float64, device="cuda")
    print(f"tomo_update K_tot={K} G=2  us (median, min, max): %.1f %.1f %.1f" % timed({"u": lambda: tomo.update(s, 0.5, out=u)})["u"])


if __name__ == "__main__":
    main()
