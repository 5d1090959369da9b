"""Time per aog_predictor_update at B = 1024, A = 64, order 2 and 4 (profiles/predictive_controller.md): HIP events around 100 launches,
after a warm-up, 7 rounds (median, min, max), then events around single launches; one JSON line per order with the bytes the update must
move (16 n^2 + 16 n A per env), the bytes the kernel form moves and the resulting share of the HBM roof."""
import json, math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from adaptive_optics_gym_amd.predictor import DevicePredictor

res = []
for order in (2, 4):
    B, A = 1024, 64
    n = A * order
    dev = DevicePredictor(B, A, order, 0.999, 1e3, 1.5e-6 / (2 * math.pi), device="cuda:0")
    g = torch.Generator("cuda").manual_seed(1)
    ys = [1e-7 * torch.randn((B, A), dtype=torch.float64, device="cuda", generator=g) for _ in range(8)]
    pred, innov = torch.empty_like(ys[0]), torch.empty_like(ys[0])
    for k in range(order + 30):
        dev.update(ys[k % 8], out=(pred, innov))
    torch.cuda.synchronize()
    rounds = []
    K = 100
    for r in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            dev.update(ys[k % 8], out=(pred, innov))
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) * 1e3 / K)
    # single launches too (events around ONE launch)
    singles = []
    for k in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dev.update(ys[k % 8], out=(pred, innov)); e1.record()
        torch.cuda.synchronize()
        singles.append(e0.elapsed_time(e1) * 1e3)
    must = B * (16 * n * n + 16 * n * A)
    moved = B * ((16 if n <= 128 else 24) * (n * n + n * A))
    us = float(np.median(rounds))
    row = dict(order=order, n=n, us_per_update_median=us, us_min=float(min(rounds)), us_max=float(max(rounds)), single_launch_us_median=float(np.median(singles)),
               must_move_bytes=must, kernel_moves_bytes=moved, must_TBps=must / us / 1e6, frac_of_8TBps=must / us / 1e6 / 8.0, frac_of_6p29TBps=must / us / 1e6 / 6.29,
               finite=bool(torch.isfinite(pred).all()))
    print(json.dumps(row), flush=True)
    res.append(row)
    dev.close()
