"""Throughput of the batched rollout (policy query + env step + bookkeeping), config-2 shaped by default; --atm dynamic --vel 10 gives the
config-4 shape, --fused-policy the causal policy stepping (epilogue + policy query + next prologue in one launch per step).  DDPG's exploration
noise (main.py:218-220: mu 0, theta 0.3, sigma 0.05): --ou advances a DeviceOUNoise inside the HIP policy query, --torch-ou adds the torch
OrnsteinUhlenbeckNoise between the query and the step (APIs the causal-stepping release already has, so this script can time it too)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from adaptive_optics_gym_amd import BatchedAOEnv
from adaptive_optics_gym_amd.rollout import DeviceActor, make_actor, rollout
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024); ap.add_argument("--N", type=int, default=256); ap.add_argument("--A", type=int, default=64)
ap.add_argument("--o", type=int, default=2); ap.add_argument("--T", type=int, default=30); ap.add_argument("--episodes", type=int, default=10)
ap.add_argument("--hidden", type=int, default=150); ap.add_argument("--actor", default="auto")
ap.add_argument("--atm", choices=("quasi_static", "dynamic"), default="quasi_static"); ap.add_argument("--vel", type=float, default=10.0)
ap.add_argument("--fused-policy", action="store_true"); ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--ou", action="store_true"); ap.add_argument("--torch-ou", action="store_true")
args = ap.parse_args()
if args.ou and args.torch_ou:
    ap.error("--ou and --torch-ou exclude each other")
dev = torch.device("cuda:0")
if args.atm == "dynamic":
    env = BatchedAOEnv(args.B, dev, atm_type="dynamic", atm_vel=args.vel, atm_fried=0.15, num_pupil_pixels=args.N, act_dim=args.A, obs_dim=args.o,
                       act_type="num_actuators", timesteps_per_episode=args.T, seed=1234, screen_source="device", screen_oversampling=16, verbose=False)
else:
    g = torch.Generator(dev).manual_seed(1)
    scr = torch.nn.functional.interpolate(torch.randn(args.B, 1, 16, 16, device=dev, generator=g), size=(args.N, args.N), mode="bicubic").squeeze(1) * 2e-6
    env = BatchedAOEnv(args.B, dev, num_pupil_pixels=args.N, act_dim=args.A, obs_dim=args.o, act_type="num_actuators", timesteps_per_episode=args.T,
                       screens=scr, verbose=False)
actor = make_actor(args.o ** 2, args.A, args.hidden, device=dev)
kw = {} if args.actor == "auto" else {"actor_impl": args.actor}
if args.fused_policy:
    kw.update(actor_impl="hip", dev_actor=DeviceActor(actor, seed=10), fused_policy=True)
if args.ou:
    from adaptive_optics_gym_amd.rollout import DeviceOUNoise
    kw["ou_noise"] = DeviceOUNoise(args.B, args.A, 0.0, 0.3, 0.05, device=dev)
elif args.torch_ou:
    from adaptive_optics_gym_amd.rollout import OrnsteinUhlenbeckNoise
    kw["ou_noise"] = OrnsteinUhlenbeckNoise(args.B, args.A, 0.0, 0.3, 0.05, device=dev)
rollout(env, actor, 1, **kw); torch.cuda.synchronize()
for rep in range(args.repeats):
    t0 = time.perf_counter()
    out = rollout(env, actor, args.episodes, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"rollout B={args.B} atm={args.atm} T={args.T} episodes={args.episodes} actor={args.actor} fused_policy={args.fused_policy} "
          f"ou={'device' if args.ou else 'torch' if args.torch_ou else 'none'} "
          f"repeat {rep}: {args.B*args.T*args.episodes/dt/1e6:.3f} M env-steps/s ({dt/(args.T*args.episodes)*1e6:.1f} us per step), "
          f"avg_ep_rew {out['avg_ep_rew']:.3f}", flush=True)
