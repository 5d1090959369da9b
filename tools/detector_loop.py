"""Step time with and without the photodetector model of the observations (aog_set_detector), on three workloads:
  config2   B = 1024, N = 256, A = 64, o = 2, quasi-static, plain step()                       (bench.py's flagship shape)
  config4   the same shape over a dynamic atmosphere (10 m/s) with the fused policy tail: reset_with_policy / step_with_policy
  o32       B = 1024, N = 256, A = 64, o = 32, quasi-static (separable route: k_obs_pass2)
Each is timed by device events around blocks of steps after a warm-up, once without a detector and once with
obs_photons = 1e4, obs_read_noise = 2; one JSON line per (workload, detector).  For per-kernel times run the same command under
``rocprofv3 --kernel-trace --stats -- python tools/detector_loop.py ...`` (in a run of its own: the trace costs time per launch)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adaptive_optics_gym_amd import BatchedAOEnv  # noqa: E402
from adaptive_optics_gym_amd.rollout import DeviceActor, make_actor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", nargs="+", default=["config2", "config4", "o32"])
ap.add_argument("--detector", nargs="+", default=["off", "on"])
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--N", type=int, default=256)
ap.add_argument("--A", type=int, default=64)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--block", type=int, default=20, help="steps between two event records (config4: one episode of 20 steps)")
ap.add_argument("--photons", type=float, default=1e4)
ap.add_argument("--read-noise", type=float, default=2.0)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator(dev).manual_seed(1)
a = torch.randn(args.B, args.A, device=dev, generator=g) * 0.7071
SHAPES = {"config2": dict(obs_dim=2), "config4": dict(obs_dim=2, atm_type="dynamic", atm_vel=10, atm_fried=0.15), "o32": dict(obs_dim=32)}

for name in args.workloads:
    for det in args.detector:
        kw = dict(SHAPES[name])
        fused = name == "config4"
        T = args.block if fused else 10 ** 9
        if det == "on":
            kw.update(obs_photons=args.photons, obs_read_noise=args.read_noise)
        env = BatchedAOEnv(args.B, dev, num_pupil_pixels=args.N, act_dim=args.A, timesteps_per_episode=T, seed=1234, verbose=False, **kw)
        if fused:
            torch.manual_seed(10)
            actor = make_actor(kw["obs_dim"] ** 2, args.A, 150, device=dev)
            pol = DeviceActor(actor, seed=10)

            def block(n):
                env.reset_with_policy(pol)
                for _ in range(n):
                    env.step_with_policy(pol)
        else:
            env.reset()

            def block(n):
                for _ in range(n):
                    env.step(a)
        for _ in range(max(1, args.warmup // args.block)):
            block(args.block)
        torch.cuda.synchronize()
        per_block, done = [], 0
        while done < args.steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            block(args.block)
            e1.record()
            e1.synchronize()
            per_block.append(e0.elapsed_time(e1) / args.block)
            done += args.block
        per_block.sort()
        med = per_block[len(per_block) // 2]
        print(json.dumps({"workload": name, "detector": det, "route": env.obs_route, "B": args.B, "N": args.N, "o": kw["obs_dim"],
                          "stepping": "reset_with_policy + step_with_policy (a reset per block)" if fused else "step",
                          "steps": done, "us_per_step_median": round(1e3 * med, 2), "us_per_step_min": round(1e3 * per_block[0], 2),
                          "us_per_step_max": round(1e3 * per_block[-1], 2), "Menv_steps_per_s": round(args.B / med / 1e3, 3),
                          "status": env.device_status()}), flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()
