"""Time ``aog_output_gradient`` at config 2's shape (1024 envs, 256 x 256 pupil, 64 modes, o = 2) next to the fused forward kernel, in one
process: HIP events over the gradient calls after warm-up, ``aog_profile_read`` for the fused kernel.  Prints one JSON line.

    python tools/time_gradient.py [--calls 200] [--warmup 50] [--envs 1024]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--envs", type=int, default=1024)
    args = ap.parse_args()
    import torch

    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A, N, T = args.envs, 64, 256, 30
    env = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_vel=0, atm_fried=0.20, act_type="num_actuators", act_dim=A, obs_dim=2,
                       timesteps_per_episode=T, num_pupil_pixels=N, seed=1234, screen_source="device", screen_oversampling=16, verbose=False)
    actions = torch.randn((T, B, A), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(10)) * (0.5 ** 0.5)
    env.reset()
    one = torch.ones(B, dtype=torch.float64, device="cuda:0")
    gobs = torch.ones((B, 4), dtype=torch.float64, device="cuda:0")
    for t in range(args.warmup):
        env.step(actions[t % T])
        env.output_gradient(gobs, one, one)
    env.profile(True, every=1, block=8)
    for t in range(args.calls):
        env.step(actions[t % T])
    torch.cuda.synchronize()
    fused_ms, n_fused = env.profile_read()
    env.profile(False)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    full_ms = timed(lambda: env.output_gradient(gobs, one, one))
    fwd_ms = timed(lambda: env.output_gradient(gobs, one, one, wrt=None, with_values=True))
    n_ap, np_ = env.tables.n_ap, (env.tables.n_ap + 31) // 32
    a_pad = 64
    # algorithmic bytes of a call: per pass the fp32 screens once (4 n_ap B) and, per env tile, the split-f16 operands of the pixel tiles
    # (modes 2 x 2 A_pad x 32, tables 2 x 2 x 32 x 32, science table 8 x 32; the backward pass the modes again as table operands)
    n_et = (B + 31) // 32
    screens = 4 * n_ap * B
    fwd_ops = np_ * (4 * a_pad * 32 + 4 * 32 * 32 + 8 * 32)
    bwd_ops = np_ * (4 * a_pad * 32 + 4 * 32 * 32 + 8 * 32 + 4 * max(a_pad, 32) * 32)
    out = dict(envs=B, n_ap=n_ap, calls=args.calls, gradient_call_ms=full_ms, forward_half_ms=fwd_ms, backward_half_ms=full_ms - fwd_ms,
               fused_forward_kernel_ms=fused_ms, fused_launches_timed=n_fused, call_over_fused=full_ms / fused_ms if fused_ms else None,
               bytes_hbm_screens=2 * screens, bytes_operands_unique=fwd_ops + bwd_ops, bytes_operands_all_env_tiles=(fwd_ops + bwd_ops) * n_et,
               device_bytes=env.device_bytes())
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
