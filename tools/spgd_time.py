"""Per-step time of rollout() loops at config 2's shape with SH_operation=True (profiles/spgd.md): wall time of 40 episodes ending in a device
synchronise over their 1200 steps, the loops of the process taking turns for five rounds after a warm-up (median, min, max) — 'spgd' fused and
unfused, the fused 'actor' step and 'ideal'.  TREE_ROOT is the checkout whose package is measured: a tree without the SPGD controller (the
commit before it) measures the last two only, so the two trees can be run in turn.  With a fourth argument: the closed-loop figure
instead — mean Strehl over the last 100 of 400 steps on a dynamic env for 'spgd', 'ideal' and 'pyramid' at two wind speeds.
usage: spgd_time.py TREE_ROOT LABEL OUT.json [closed]"""
import json
import sys
import time

root, label, out_path = sys.argv[1], sys.argv[2], sys.argv[3]
closed = len(sys.argv) > 4
sys.path.insert(0, root)
import numpy as np
import torch

import adaptive_optics_gym_amd
from adaptive_optics_gym_amd import BatchedAOEnv
from adaptive_optics_gym_amd.rollout import make_actor, rollout

assert adaptive_optics_gym_amd.__file__.startswith(root), adaptive_optics_gym_amd.__file__
try:
    from adaptive_optics_gym_amd.sensorless import SPGDController
except ImportError:
    SPGDController = None

res = {"label": label, "tree": root}
if not closed:
    B, N, A, T = 1024, 256, 64, 30
    env = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_fried=0.20, act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T,
                       SH_operation=True, rew_type="strehl_ratio", seed=3, verbose=False)
    torch.manual_seed(1)
    actor = make_actor(4, A, 150, device="cuda:0")
    with torch.no_grad():   # raw actuators in metres on this env: keep the policy's commands physical
        actor.out.weight.mul_(1e-6)
        actor.out.bias.mul_(1e-6)
    loops = {"actor_fused": lambda e: rollout(env, actor, episodes=e, actor_impl="hip", fused_policy=True, cov_var=1e-16),
             "ideal": lambda e: rollout(env, None, episodes=e, policy="ideal")}
    if SPGDController is not None:
        ctrl = SPGDController(env, gain=2e-6, amplitude=2e-8, metric="strehl", seed=7)
        loops["spgd_fused"] = lambda e: rollout(env, None, episodes=e, policy="spgd", controller=ctrl, fused_policy=True)
        loops["spgd_unfused"] = lambda e: rollout(env, None, episodes=e, policy="spgd", controller=ctrl, fused_policy=False)
    EP, ROUNDS = 40, 5
    for f in loops.values():
        f(5)
    torch.cuda.synchronize()
    times = {k: [] for k in loops}
    for r in range(ROUNDS):
        for k, f in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(EP)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (EP * T) * 1e6)
    res["shape"] = dict(B=B, N=N, A=A, T=T, episodes_per_window=EP, rounds=ROUNDS)
    res["us_per_step"] = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=v) for k, v in times.items()}
else:
    B, N, A, T = 64, 64, 16, 400
    res["closed_loop"] = {}
    for vel in (1.0, 10.0):
        row = {}
        for policy in ("spgd", "ideal", "pyramid"):
            env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=vel, atm_fried=0.15, act_dim=A, obs_dim=2, num_pupil_pixels=N,
                               timesteps_per_episode=T, SH_operation=True, rew_type="strehl_ratio", seed=11, verbose=False,
                               pyramid=dict(samples=16, pixels=16, n_mod=4, r_mod=2.0))
            kw = {}
            if policy == "spgd":
                ctrl = SPGDController(env, gain=2e-6, amplitude=2e-8, metric="strehl", seed=7)
                kw = dict(controller=ctrl, fused_policy=True)
            out = rollout(env, None, episodes=1, policy=policy, **kw)
            strehl = (out["rew"].double() + 100.0) / 100.0    # reward = -(100 - 100 Strehl)
            row[policy] = dict(mean_last100=float(strehl[-100:].mean()), mean_first10=float(strehl[:10].mean()),
                               min_env_last100=float(strehl[-100:].mean(0).min()), max_env_last100=float(strehl[-100:].mean(0).max()))
            env.close()
        res["closed_loop"]["vel_%g" % vel] = row
    res["closed_shape"] = dict(B=B, N=N, A=A, T=T, atm_fried=0.15, gain=2e-6, amplitude=2e-8)
print(json.dumps(res))
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
