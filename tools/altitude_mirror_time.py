"""Times of the altitude mirror (profiles/altitude_mirror.md).
usage: altitude_mirror_time.py calls OUT.json                  aog_altmirror_set_command and aog_altmirror_fit at B = 1024, M = 288, K = 81: HIP
                                                               events around 200 calls after a warm-up, 5 rounds (median, min, max); the counts
                                                               the kernels' rates are read against come from the shapes
       altitude_mirror_time.py step TREE_ROOT LABEL OUT.json   LayeredAOEnv.step us per step at 1024 envs, N = 64 under a meta-pupil of 88 (the largest
                                                               shape of this kind whose layers evolve: profiles/sightlines.md), two layers (0 and 10 km),
                                                               one sightline, with one 9 x 9 altitude mirror whose command is set every step and without
                                                               (a tree without AltitudeMirror, the commit before it, measures the second only): wall
                                                               time of 300 steps ending in a device synchronise, five rounds, the envs taking turns"""
import json
import os
import sys
import time

mode = sys.argv[1]
root = sys.argv[2] if mode == "step" else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, root)
import numpy as np
import torch

import adaptive_optics_gym_amd
from adaptive_optics_gym_amd import LayeredAOEnv

assert os.path.realpath(adaptive_optics_gym_amd.__file__).startswith(os.path.realpath(root)), adaptive_optics_gym_amd.__file__
try:
    from adaptive_optics_gym_amd.conjugate import AltitudeMirror
except ImportError:
    AltitudeMirror = None


def timed_in_turns(fns, calls=200, rounds=5, warm=10):
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


class _Owner:
    def __init__(self, B, N, M, device):
        self.num_envs, self.num_pupil_pixels, self.meta_pupil_pixels, self.device = B, N, M, device


res = {"mode": mode}
if mode == "calls":
    from adaptive_optics_gym_amd import BatchedAOEnv, OpticalParams
    import dataclasses

    out_path = sys.argv[2]
    B, N, M, n = 1024, 256, 288, 9
    K = n * n
    mirror = AltitudeMirror(_Owner(B, N, M, "cuda:0"), 1e4, actuators=n)
    params = dataclasses.replace(OpticalParams(num_pupil_pixels=N), num_pupil_pixels=M, telescope_diameter=0.5 * M / N)
    layer = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30.0, atm_fried=0.15, seed=3, params=params, act_type="zernike", act_dim=6, obs_dim=2,
                         num_pupil_pixels=M, timesteps_per_episode=0, verbose=False)
    # (the layer's screens as drawn: a dynamic handle of 288 pixels does not evolve — profiles/sightlines.md — and the fit reads any ring alike)
    cmd = torch.randn((B, K), dtype=torch.float64, device="cuda") * 1e-7
    some = torch.arange(B, device="cuda") % 8 == 0
    fns = {"aog_altmirror_set_command": lambda: mirror.set_command(cmd), "aog_altmirror_set_command(mask: one env in 8)": lambda: mirror.set_command(cmd, some),
           "aog_altmirror_fit": lambda: mirror.fit_layer(layer)}
    res.update(shape=dict(B=B, M=M, K=K), us_per_call=timed_in_turns(fns))
    # what the algorithm needs, from the shapes: kernel 1 one product and one sum per (env, mode, pixel) less the first sum, the surfaces written once
    # and the basis read at least once; kernel 2 one fma per (env, mode, pixel), the screens and the fit matrix read at least once
    MM = M * M
    res["counts"] = {"surface_flop": B * MM * (2 * K - 1), "surface_bytes_min": 8 * (B * MM + K * MM + B * K), "surface_basis_bytes_requested": 8 * K * MM * ((B + 7) // 8),
                     "fit_flop": 2 * B * K * MM, "fit_bytes_min": 8 * (B * MM + K * MM), "fit_matrix_bytes_requested": 8 * K * MM * B}
    mirror.close(), layer.close()
else:
    label, out_path = sys.argv[3], sys.argv[4]
    B, N, A, T = 1024, 64, 16, 30
    kw = dict(atm_layers=[{"fraction": 0.6, "speed": 10.0}, {"fraction": 0.4, "speed": 30.0}], atm_fried=0.15, act_dim=A, obs_dim=2, num_pupil_pixels=N,
              timesteps_per_episode=T, rew_type="strehl_ratio", seed=3, verbose=False, layer_altitudes=[0.0, 1e4], meta_pupil_pixels=88, sightlines={"uplink": (8e-6, 0.0)})
    envs = {"sightline": LayeredAOEnv(B, "cuda:0", **kw)}
    if AltitudeMirror is not None:
        envs["sightline_mirror"] = LayeredAOEnv(B, "cuda:0", altitude_mirrors=[dict(altitude=1e4, actuators=9)], **kw)
    acts = torch.randn((B, A), device="cuda") * 0.5
    cmd = torch.randn((B, 81), dtype=torch.float64, device="cuda") * 1e-7

    def loop(env, steps):
        for t in range(steps):
            if t % T == 0:
                env.reset()
            if getattr(env, "altitude_mirrors", None):
                env.altitude_mirrors[0].set_command(cmd)
            env.step(acts)

    STEPS, ROUNDS = 300, 5
    for env in envs.values():
        loop(env, 10)
    torch.cuda.synchronize()
    times = {k: [] for k in envs}
    for r in range(ROUNDS):
        for k, env in envs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(env, STEPS)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / STEPS * 1e6)
    res.update(label=label, tree=root, shape=dict(B=B, N=N, A=A, T=T, meta_pupil_pixels=int(envs["sightline"].meta_pupil_pixels), steps_per_window=STEPS, rounds=ROUNDS))
    res["us_per_step"] = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=v) for k, v in times.items()}
    for env in envs.values():
        env.close()
print(json.dumps(res))
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
