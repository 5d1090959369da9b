"""Timing loop of the layered atmosphere (profiles/layered_atmosphere.md): per-step device time of a LayeredAOEnv with L = 1, 2, 3 layers,
the time of aog_install_layer_sum alone and the bytes it moves per second, beside the plain single-layer dynamic env of the same shape.

    python tools/layered_loop.py [--envs 1024] [--pupil 256] [--steps 200] [--warmup 20] [--layers 1 2 3]

Device time is HIP-event time over `steps` back-to-back calls after `warmup` (no host synchronisation inside the window)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--pupil", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM roof the achieved bytes/s are compared with (GB/s)")
    a = ap.parse_args()
    import torch

    from adaptive_optics_gym_amd import BatchedAOEnv, LayeredAOEnv

    B, N, A = a.envs, a.pupil, 64
    kw = dict(act_type="num_actuators", act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=10 ** 9, num_pupil_pixels=N, seed=1234,
              verbose=False)
    acts = torch.randn((B, A), device="cuda") * 0.5 ** 0.5
    plain = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=10, atm_fried=0.15, **kw)
    plain.reset()
    row = {"config": "plain dynamic", "envs": B, "pupil": N, "step_us": timed(torch, lambda: plain.step(acts), a.steps, a.warmup),
           "evolve_us": timed(torch, plain.evolve_atmosphere, a.steps, a.warmup)}
    print(json.dumps(row), flush=True)
    tables = plain.tables
    plain.close()
    speeds, fractions = [5.0, 10.0, 20.0], {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.3, 0.2]}
    for L in a.layers:
        env = LayeredAOEnv(B, "cuda:0", atm_layers=[{"fraction": f, "speed": v} for f, v in zip(fractions[L], speeds)], atm_fried=0.15, tables=tables, **kw)
        env.reset()
        step_us = timed(torch, lambda: env.step(acts), a.steps, a.warmup)
        install_us = timed(torch, env._install, a.steps, a.warmup)
        evolve_us = timed(torch, lambda: [lay.evolve_atmosphere() for lay in env.layers], a.steps, a.warmup)
        n_ap = int(env.tables.n_ap)
        # both passes read 8 n_ap bytes per env and layer; the second writes the fp32 tiles (padding included)
        moved = 2 * 8 * n_ap * B * L + 4 * env.info.num_envs_padded * env.info.n_ap_padded
        row = {"config": f"layered L={L}", "envs": B, "pupil": N, "step_us": step_us, "install_us": install_us, "evolve_us": evolve_us,
               "install_bytes": moved, "install_gbs": moved / install_us * 1e-3, "hbm_fraction": moved / install_us * 1e-3 / a.hbm_gbs}
        print(json.dumps(row), flush=True)
        env.close()


if __name__ == "__main__":
    main()
