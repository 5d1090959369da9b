"""Times and a closed-loop figure of the mirror servo (profiles/servo.md).
usage: servo_time.py calls OUT.json                     one aog_servo_apply at B = 1024, A = 64 with latency 1.5 and response 0.5 against the same
                                                        arithmetic in eager torch on the same tensors: HIP events around 5000 calls after a
                                                        warm-up, 5 rounds (median, min, max), the two taking turns; the results compared
                                                        (under a kernel trace the same run gives k_servo_apply's own duration)
       servo_time.py rollout TREE_ROOT LABEL OUT.json   rollout(policy='ideal') us per step at config 2's shape with servo=dict(latency=1.5,
                                                        response=0.5) and without (a tree without MirrorServo, the commit before it, measures the
                                                        second only): wall time of 40 episodes ending in a device synchronise, five rounds
       servo_time.py closed OUT.json                    residual rms of 'ideal' and 'predictive' at total loop delay 1, 2 and 3 frames (servo
                                                        latency 0, 1, 2), dynamic atmosphere"""
import json
import os
import sys
import time

mode = sys.argv[1]
root = sys.argv[2] if mode == "rollout" else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, root)
import numpy as np
import torch

import adaptive_optics_gym_amd
from adaptive_optics_gym_amd import BatchedAOEnv
from adaptive_optics_gym_amd.rollout import rollout

assert os.path.realpath(adaptive_optics_gym_amd.__file__).startswith(os.path.realpath(root)), adaptive_optics_gym_amd.__file__
try:
    from adaptive_optics_gym_amd.servo import MirrorServo
except ImportError:
    MirrorServo = None


def timed_in_turns(fns, calls=5000, rounds=5, warm=50):
    """Microseconds per call of each function: HIP events around `calls` calls, `rounds` rounds after a warm-up, the functions taking turns."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in us.items()}


class EagerServo:
    """The same arithmetic in eager torch, as a user would write it: a ring of the last commands, the interpolated read, the response."""

    def __init__(self, B, A, latency, response, depth, device):
        self.d, self.f, self.r, self.R = int(latency), float(latency) - int(latency), float(response), depth
        self.ring = torch.zeros((depth, B, A), dtype=torch.float32, device=device)
        self.y = torch.zeros((B, A), dtype=torch.float64, device=device)
        self.n = 0

    def apply(self, a):
        R, n = self.R, self.n
        self.ring[n % R].copy_(a)
        c = (1.0 - self.f) * self.ring[(n - self.d) % R].double() + self.f * self.ring[(n - self.d - 1) % R].double()
        self.y = self.y + self.r * (c - self.y)
        self.n += 1
        return self.y.float()


class _Batch:
    def __init__(self, B, A, device):
        self.num_envs, self.num_modes, self.global_env_offset, self.total_envs, self.device = B, A, 0, B, device


res = {"mode": mode}
if mode == "calls":
    out_path = sys.argv[2]
    B, A, LAT, RESP = 1024, 64, 1.5, 0.5
    dev = torch.device("cuda", 0)
    servo = MirrorServo(_Batch(B, A, dev), latency=LAT, response=RESP)
    eager = EagerServo(B, A, LAT, RESP, servo.max_latency + 2, dev)
    gen = torch.Generator("cuda").manual_seed(1)
    acts = torch.randn((8, B, A), device="cuda", generator=gen)
    worst = 0.0
    for t in range(8):   # the two agree (the eager form's rounding is torch's business: held to 1e-6, a few float32 steps of a unit action)
        worst = max(worst, float((servo.apply(acts[t]) - eager.apply(acts[t])).abs().max()))
    assert worst <= 1e-6, f"aog_servo_apply and the eager form differ by {worst}"
    out = torch.empty((B, A), dtype=torch.float32, device="cuda")
    turn = [0]

    def kernel():
        turn[0] = (turn[0] + 1) % 8
        servo.apply(acts[turn[0]], out=out)

    def in_torch():
        turn[0] = (turn[0] + 1) % 8
        eager.apply(acts[turn[0]])

    res.update(shape=dict(B=B, A=A, latency=LAT, response=RESP), max_abs_difference=worst, us_per_call=timed_in_turns({"aog_servo_apply": kernel, "eager_torch": in_torch}))
    # bytes one call moves: the action in, the ring slot written and two read, y read and written, the stuck bytes and values, the action out
    moved = B * A * (4 + 4 + 8 + 16 + 1 + 4 + 4)
    res.update(bytes_per_call=moved, us_at_8TBps=moved / 8e6)
    servo.close()
elif mode == "rollout":
    label, out_path = sys.argv[3], sys.argv[4]
    B, N, A, T = 1024, 256, 64, 30
    kw = dict(atm_type="quasi_static", atm_fried=0.20, act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T, SH_operation=True,
              rew_type="strehl_ratio", seed=3, verbose=False)
    envs = {"ideal": BatchedAOEnv(B, "cuda:0", **kw)}
    if MirrorServo is not None:
        envs["ideal_servo"] = BatchedAOEnv(B, "cuda:0", servo=dict(latency=1.5, response=0.5), **kw)
    loops = {k: (lambda e, env=env: rollout(env, None, episodes=e, policy="ideal")) for k, env in envs.items()}
    EP, ROUNDS = 40, 5
    for fn in loops.values():
        fn(5)
    torch.cuda.synchronize()
    times = {k: [] for k in loops}
    for r in range(ROUNDS):
        for k, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(EP)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (EP * T) * 1e6)
    res.update(label=label, tree=root, shape=dict(B=B, N=N, A=A, T=T, episodes_per_window=EP, rounds=ROUNDS))
    res["us_per_step"] = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=v) for k, v in times.items()}
else:
    from adaptive_optics_gym_amd.predictor import PredictiveController

    out_path = sys.argv[2]
    B, N, A, T = 64, 64, 16, 1024
    res["closed_shape"] = dict(B=B, N=N, A=A, steps=T, atm_fried=0.1, atm_vel=10.0, skipped=256)
    for delay in (1, 2, 3):
        row = {}
        for policy in ("ideal", "predictive"):
            env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=10.0, atm_fried=0.1, act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T,
                               SH_operation=True, rew_type="strehl_ratio", seed=11, verbose=False, **({} if delay == 1 else {"servo": dict(latency=delay - 1)}))
            ctrl = PredictiveController(env) if policy == "predictive" else None
            env.reset()
            rms, fit, strehl = [], [], []
            for t in range(T):
                a = ctrl.action() if ctrl is not None else env.ideal_action()
                r = env.step(a.to(torch.float32))
                if t >= 256:   # (the predictor has learnt by then; the same window for both)
                    w = env.wavefront_truth()
                    rms.append(w["rms"].clone()), fit.append(w["fit_rms"].clone()), strehl.append(r[4]["strehl"].clone())
            rms, fit = torch.stack(rms).double(), torch.stack(fit).double()
            row[policy] = dict(residual_rms_nm=float((rms ** 2).mean().sqrt() * 1e9), fit_rms_nm=float((fit ** 2).mean().sqrt() * 1e9),
                               servo_lag_rms_nm=float(((rms ** 2).mean() - (fit ** 2).mean()).clamp_min(0).sqrt() * 1e9),
                               mean_strehl=float(torch.stack(strehl).double().mean()))
            env.close()
        res["delay%d" % delay] = row
print(json.dumps(res))
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
