"""Times and a closed-loop figure of the LQG controller (profiles/lqg.md).
usage: lqg_time.py calls OUT.json    one aog_lqg_update and one aog_lqg_solve (256 iterations) at B = 1024, A = 64 with S = 2 and S = 4, beside
                                     ModalIntegrator.update (eager torch) on the same measurements: HIP events around the calls after a warm-up,
                                     5 rounds (median, min, max), the three taking turns; and the bytes an update must move
       lqg_time.py closed OUT.json   residual rms on the vibrating mode for 'modal' after retune(), 'predictive', 'lqg' and 'lqg' after
                                     identify() on a LayeredAOEnv with a vibration line on tip (N = 32, B = 4, A = 9, two layers): 1024 steps,
                                     the first 256 dropped, with and without servo=dict(latency=1)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from adaptive_optics_gym_amd import LayeredAOEnv, LQGController, ModalIntegrator, ModalTelemetry
from adaptive_optics_gym_amd.lqg import DeviceLQG, default_model
from adaptive_optics_gym_amd.params import OpticalParams
from adaptive_optics_gym_amd.predictor import PredictiveController

mode, out_path = sys.argv[1], sys.argv[2]


def timed_in_turns(fns, calls, rounds=5, warm=20):
    """Microseconds per call of each function: HIP events around `calls[k]` calls, `rounds` rounds after a warm-up, the functions taking turns."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[k]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / calls[k])
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in us.items()}


class _Batch:
    def __init__(self, B, A, device):
        self.num_envs, self.num_modes, self.global_env_offset, self.device, self.pyramid = B, A, 0, device, None


res = {"mode": mode}
if mode == "calls":
    B, A = 1024, 64
    dev = torch.device("cuda", 0)
    gen = torch.Generator("cuda").manual_seed(1)
    ys = torch.randn((8, B, A), device="cuda", generator=gen, dtype=torch.float64)
    out = torch.empty((B, A), dtype=torch.float64, device="cuda")
    turn = [0]
    res["shape"] = dict(B=B, A=A, iterations=256)
    for S in (2, 4):
        line = dict(frequency=0.12, damping=0.01, ratio=0.25)
        a, q, r, _ = default_model(B, A, [dict(line, frequency=0.12 + 0.05 * k) for k in range(S - 1)])
        f = DeviceLQG(B, A, S, device=dev)
        f.set_model(*(torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous() for v in (a, q, r)))
        conv = f.solve(1, 256)
        assert float(conv.max()) <= 1e-9, float(conv.max())
        integ = ModalIntegrator(_Batch(B, A, dev), telemetry=ModalTelemetry(B, A, length=64, device=dev))
        integ.telemetry.push = lambda y, mask=None: None   # the integrator's own arithmetic alone (the LQG call timed here pushes nothing either)

        def update():
            turn[0] = (turn[0] + 1) % 8
            f.update(ys[turn[0]], out=out)

        def solve():
            f.solve(1, 256, out=out)

        def modal():
            turn[0] = (turn[0] + 1) % 8
            integ.update(ys[turn[0]])

        us = timed_in_turns({"aog_lqg_update": update, "aog_lqg_solve": solve, "ModalIntegrator.update": modal},
                            {"aog_lqg_update": 2000, "aog_lqg_solve": 50, "ModalIntegrator.update": 500})
        n = 2 * S
        # what one update must move per (env, mode), 8 bytes each: y, xhat read and written, K, c_d, a1 and a2, the command and out written
        moved = B * A * 8 * (1 + 2 * n + n + n + 2 * S + 2)
        res[f"S{S}"] = dict(us_per_call=us, update_bytes=moved, update_us_at_8TBps=moved / 8e6, update_us_at_6p29TBps=moved / 6.29e6)
        f.close()
else:
    N, B, A, T, SKIP = 32, 4, 9, 1024, 256
    dt = float(OpticalParams(num_pupil_pixels=N).delta_t)
    line = dict(frequency=0.12, damping=0.01)
    res["closed_shape"] = dict(N=N, B=B, A=A, steps=T, skipped=SKIP, line=dict(line, rms_m=5e-8, shape="tip"), lqg_ratio=1.0)
    for latency in (0, 1):
        row = {}
        for policy in ("modal", "predictive", "lqg", "lqg_identified"):
            kw = dict(atm_layers=[{"fraction": 0.6, "speed": 10.0}, {"fraction": 0.4, "speed": 15.0}], atm_fried=0.15, seed=11, act_type="zernike", act_dim=A,
                      obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T, num_pupil_pixels=N, verbose=False, SH_operation=True,
                      disturbance=dict(shapes=["tip"], vibrations=[dict(term=0, frequency=line["frequency"] / dt, damping=line["damping"], rms=5e-8)]))
            if latency:
                kw["servo"] = dict(latency=latency)
            env = LayeredAOEnv(B, "cuda:0", **kw)
            mode_j = int(np.argmax(np.abs(np.asarray(env.tables.modes).T @ env.disturbance.basis[0])))
            delay = 1 + latency
            if policy == "modal":
                ctrl = ModalIntegrator(env, delay=delay, gain=0.3)
            elif policy == "predictive":
                ctrl = PredictiveController(env)
            else:
                ctrl = LQGController(env, delay=delay, vibrations=[dict(line, ratio=1.0)])
            env.reset()
            coef, extra = [], {}
            for t in range(T):
                if t == SKIP and policy == "modal":
                    ctrl.retune()
                    extra["gain_on_the_mode"] = ctrl.gains[:, mode_j].tolist()
                if t == SKIP and policy == "lqg_identified":
                    valid = ctrl.identify()
                    try:
                        ctrl.solve()
                    except ValueError as err:   # (reported, not hidden: the run of this policy ends here)
                        extra["solve_error"] = str(err)
                        break
                    extra["valid_fraction"] = float(valid.double().mean())
                    extra["turbulence_roots_on_the_mode"] = [np.abs(np.roots([1.0, -float(ctrl.a[b, 0, 0, mode_j]), -float(ctrl.a[b, 0, 1, mode_j])])).tolist()
                                                             for b in range(B)]
                env.step(ctrl.action().to(torch.float32))
                if t >= SKIP:
                    coef.append(env.wavefront_truth()["coef"].clone())
            if not coef:
                row[policy] = extra
                ctrl.close(), env.close()
                continue
            coef = torch.stack(coef).double()   # [T - SKIP, B, A] metres: the residual's modal coefficients
            row[policy] = dict(residual_rms_on_the_mode_nm=float((coef[:, :, mode_j] ** 2).mean().sqrt() * 1e9),
                               residual_rms_all_modes_nm=float((coef ** 2).sum(dim=2).mean().sqrt() * 1e9), mode=mode_j, **extra)
            ctrl.close()
            env.close()
        res["latency%d" % latency] = row
print(json.dumps(res))
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
