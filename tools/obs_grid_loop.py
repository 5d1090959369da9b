"""Step time against the observation size: B = 1024, N = 256, A = 64, quasi-static, o in {5, 8, 16, 32} by default (o = 5 takes the table
route, the others the separable matrix-core route).  step() is timed by device events around blocks of steps on the current stream, after a
warm-up; one JSON line per o.  For a kernel table run the same command under ``rocprofv3 --kernel-trace --stats -- python tools/obs_grid_loop.py``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adaptive_optics_gym_amd import BatchedAOEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--N", type=int, default=256)
ap.add_argument("--A", type=int, default=64)
ap.add_argument("--o", type=int, nargs="+", default=[5, 8, 16, 32])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--block", type=int, default=50, help="steps between two event records")
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator(dev).manual_seed(1)
# smooth synthetic screens (a few rad rms): no kernel's cost depends on their spectrum
scr = torch.nn.functional.interpolate(torch.randn(args.B, 1, 16, 16, device=dev, generator=g), size=(args.N, args.N), mode="bicubic").squeeze(1) * 2e-6
a = torch.randn(args.B, args.A, device=dev, generator=g) * 0.7071
for o in args.o:
    env = BatchedAOEnv(args.B, dev, num_pupil_pixels=args.N, act_dim=args.A, obs_dim=o, timesteps_per_episode=10 ** 9, screens=scr, verbose=False)
    env.reset()
    for _ in range(args.warmup):
        env.step(a)
    torch.cuda.synchronize()
    per_block = []
    done = 0
    while done < args.steps:
        nb = min(args.block, args.steps - done)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(nb):
            env.step(a)
        e1.record()
        e1.synchronize()
        per_block.append(e0.elapsed_time(e1) / nb)
        done += nb
    per_block.sort()
    med = per_block[len(per_block) // 2]
    print(json.dumps({"o": o, "route": env.obs_route, "B": args.B, "N": args.N, "A": args.A, "steps": args.steps,
                      "ms_per_step_median": round(med, 4), "ms_per_step_min": round(per_block[0], 4), "ms_per_step_max": round(per_block[-1], 4),
                      "Menv_steps_per_s": round(args.B / med / 1e3, 3), "status": env.device_status()}), flush=True)
    env.close()
    del env
    torch.cuda.empty_cache()
