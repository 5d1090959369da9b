"""Time per aog_telemetry_psd and aog_telemetry_gains call at B = 1024, A = 64, T = 512, S = 128 (profiles/telemetry.md): HIP events around
20 launches after a warm-up, 7 rounds (median, min, max), then events around single launches.  Two handles take turns so that no call
finds its 268 MB ring in the Infinity Cache from the call before.  One JSON line per call with the bytes it must move (the ring once plus
its outputs) and the resulting share of the HBM roof."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from adaptive_optics_gym_amd.telemetry import ModalTelemetry, default_grid

B, A, T, S, G = 1024, 64, 512, 128, 32
tels = [ModalTelemetry(B, A, length=T, device="cuda:0") for _ in range(2)]
g = torch.Generator("cuda").manual_seed(1)
ys = [1e-7 * torch.randn((B, A), dtype=torch.float64, device="cuda", generator=g) for _ in range(8)]
for k in range(T + 17):
    for t in tels:
        t.push(ys[(k * 5 + k // 8) % 8])
grid = default_grid(1)
NB = S // 2 + 1
ring = B * T * A * 8
calls = {"psd": (lambda t: t.psd(S), ring + B * A * NB * 8 + B * 4), "gains": (lambda t: t.optimise_gains(1, grid, S), ring + 2 * B * A * 8),
         "gains_with_costs": (lambda t: t.optimise_gains(1, grid, S, with_costs=True), ring + (2 + G) * B * A * 8)}
for name, (fn, must) in calls.items():
    for k in range(6):
        out = fn(tels[k % 2])
    torch.cuda.synchronize()
    rounds, K = [], 20
    for r in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            out = fn(tels[k % 2])
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) * 1e3 / K)
    singles = []
    for k in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(tels[k % 2]); e1.record()
        torch.cuda.synchronize()
        singles.append(e0.elapsed_time(e1) * 1e3)
    us = float(np.median(rounds))
    print(json.dumps(dict(call=name, B=B, A=A, T=T, S=S, us_per_call_median=us, us_min=float(min(rounds)), us_max=float(max(rounds)),
                          single_launch_us_median=float(np.median(singles)), must_move_bytes=must, must_TBps=must / us / 1e6,
                          frac_of_8TBps=must / us / 1e6 / 8.0, us_at_8TBps=must / 8e6, finite=bool(torch.isfinite(out[1]).all()))), flush=True)
# the push, for scale
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for k in range(200):
    tels[0].push(ys[k % 8])
e1.record()
torch.cuda.synchronize()
print(json.dumps(dict(call="push", us_per_call=e0.elapsed_time(e1) * 1e3 / 200)), flush=True)
