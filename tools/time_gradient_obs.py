"""Time ``aog_output_gradient`` with the observation gradient of the separable route (``obs_gradient=True``) at 1024 envs, a 256 x 256
pupil and 64 modes, for o = 8 and 32, in one process per o: HIP events over the calls after warm-up — the call with ``g_obs``, the same
handle's call with ``g_obs=None``, the forward half alone (the values) and the env's own step.  Prints one JSON line per o.

    python tools/time_gradient_obs.py [--calls 200] [--warmup 20] [--envs 1024] [--obs-dims 8 32]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--obs-dims", type=int, nargs="+", default=[8, 32])
    args = ap.parse_args()
    import torch

    from adaptive_optics_gym_amd import BatchedAOEnv

    B, A, N, T = args.envs, 64, 256, 30
    for o in args.obs_dims:
        env = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_vel=0, atm_fried=0.20, act_type="num_actuators", act_dim=A, obs_dim=o,
                           timesteps_per_episode=T, num_pupil_pixels=N, seed=1234, screen_source="device", screen_oversampling=16, verbose=False,
                           obs_gradient=True)
        actions = torch.randn((T, B, A), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(10)) * (0.5 ** 0.5)
        env.reset()
        one = torch.ones(B, dtype=torch.float64, device="cuda:0")
        gobs = torch.randn((B, o * o), dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(11))
        for t in range(args.warmup):
            env.step(actions[t % T])
            env.output_gradient(gobs, one, one, with_values=True)
            env.output_gradient(None, one, one)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.calls):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.calls

        step_ms = timed(lambda i: env.step(actions[i % T]))
        full_ms = timed(lambda i: env.output_gradient(gobs, one, one))
        obs_only_ms = timed(lambda i: env.output_gradient(gobs, None, None))
        tab_ms = timed(lambda i: env.output_gradient(None, one, one))
        values_ms = timed(lambda i: env.output_gradient(None, one, one, wrt=None, with_values=True))
        print(json.dumps(dict(envs=B, n_pupil=N, modes=A, obs_dim=o, n_ap=env.tables.n_ap, calls=args.calls, step_ms=step_ms,
                              call_g_obs_power_strehl_ms=full_ms, call_g_obs_alone_ms=obs_only_ms, call_without_g_obs_ms=tab_ms,
                              values_alone_ms=values_ms, device_bytes=env.device_bytes())), flush=True)
        env.close()


if __name__ == "__main__":
    main()
