#!/usr/bin/env python3
"""Cost of the science camera on the device: ``science_integrate`` of a whole batch at two windows against ``focal_images`` (K4: the same
pass structure with 128^2 outputs) in one process, alternated, timed with device events.  Prints one JSON line per case and a summary:
time per call, matrix instructions per env (v_mfma_f32_32x32x16_f16, 12 per complex 32x32x16 tile product) and the achieved matrix rate.

    python tools/science_camera_cost.py [--envs 1024] [--pupil 256] [--modes 64] [--trials 7] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP_PER_MFMA = 2 * 32 * 32 * 16


def up(v, m):
    return (v + m - 1) // m * m


def mfma_per_env(N, rows_blocks, cols_blocks):
    """pass 1: (Nxp / 32 x tiles) x (row blocks) x (Nyp / 16 k-steps); pass 2: (row blocks) x (column blocks) x (Nxp / 16 k-steps); 12 each."""
    Nxp, Nyp = up(N, 128), up(N, 16)
    return 12 * ((Nxp // 32) * rows_blocks * (Nyp // 16) + rows_blocks * cols_blocks * (Nxp // 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--pupil", type=int, default=256)
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch

    from adaptive_optics_gym_amd import BatchedAOEnv

    if not torch.cuda.is_available():
        raise SystemExit("science_camera_cost.py needs a HIP device: nothing is measured without one")
    B, N, A = args.envs, args.pupil, args.modes
    kw = dict(act_dim=A, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=N, timesteps_per_episode=30, seed=1234, verbose=False)
    actions = torch.randn((B, A), device="cuda", generator=torch.Generator("cuda").manual_seed(10)) * 0.5 ** 0.5
    cases = {}
    # (AOG_SCIENCE_SPLIT is read by every integrate: the same handle is timed in both tile geometries of a two-block window)
    for name, w, split in (("science w=64, blocks shared by the waves", 64, "1"), ("science w=64, one block per wave", 64, "0"),
                           ("science w=240", 240, "1"), ("focal_images (K4, 128^2)", None, "1")):
        env = BatchedAOEnv(B, "cuda:0", science_window=w, **kw)
        env.reset()
        env.step(actions)
        if w is None:
            call, blocks = env.focal_images, (4, 4)
        else:
            call, blocks = env.science_integrate, ((w + 31) // 32,) * 2
        cases[name] = dict(env=env, call=call, mfma=mfma_per_env(N, *blocks), ms=[], split=split)
        os.environ["AOG_SCIENCE_SPLIT"] = split
        for _ in range(5):   # warm-up: code objects, work buffers of the first call
            call()
    torch.cuda.synchronize()
    for _ in range(args.trials):   # alternated: every trial times each case once
        for c in cases.values():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            os.environ["AOG_SCIENCE_SPLIT"] = c["split"]
            t0.record()
            for _ in range(args.calls):
                c["call"]()
            t1.record()
            t1.synchronize()
            c["ms"].append(t0.elapsed_time(t1) / args.calls)
    for name, c in cases.items():
        med = statistics.median(c["ms"])
        print(json.dumps({"case": name, "envs": B, "pupil": N, "ms_per_call_median": round(med, 4), "ms_min": round(min(c["ms"]), 4),
                          "ms_max": round(max(c["ms"]), 4), "mfma_per_env": c["mfma"],
                          "matrix_tflops": round(c["mfma"] * B * FLOP_PER_MFMA / (med * 1e-3) / 1e12, 1)}), flush=True)
        c["env"].close()


if __name__ == "__main__":
    main()
