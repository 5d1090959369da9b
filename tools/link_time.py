"""Times and a closed-loop figure of the link telemetry (profiles/link_telemetry.md).
usage: link_time.py calls OUT.json               one push, one statistics call at length 1024 and 4096 (B = 1024, K = 3, E = 32, Q = 2): HIP events
                                                 around 20 calls after a warm-up, 7 rounds (median, min, max); beside each the time its bytes
                                                 imply at 8 TB/s and the same statistics in eager torch on the same samples
       link_time.py rollout TREE_ROOT LABEL OUT.json   rollout(policy='ideal') steps/s at config 2's shape with and without link= (a tree
                                                 without LinkTelemetry, the commit before it, measures the second only): wall time of 40
                                                 episodes ending in a device synchronise, the loops taking turns for five rounds
       link_time.py closed OUT.json              -3 dB fade fraction and mean fade duration at r0 = 0.1 m, dynamic atmosphere, for 'ideal', 'modal'
                                                 and a flat mirror"""
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
    from adaptive_optics_gym_amd.link import LinkTelemetry, db_to_factor
except ImportError:
    LinkTelemetry = None


def timed(fn, calls=20, rounds=7, warm=6):
    """Microseconds per call: HIP events around `calls` calls, `rounds` rounds after a warm-up -> (median, min, max)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return dict(median=float(np.median(us)), min=float(min(us)), max=float(max(us)))


def eager_statistics(win, f, g, q):
    """The same figures in eager torch on chronological windows win [B, n] float32 (reference = the env's mean): what a user would write."""
    B, n = win.shape
    p = win.double()
    mean, msq = p.mean(1), (p * p).mean(1)
    below_edge = p.unsqueeze(1) < (mean.unsqueeze(1) * f).unsqueeze(2)          # [B, K, n]
    below = below_edge.sum(2)
    starts = below_edge & ~torch.nn.functional.pad(below_edge[:, :, :-1], (1, 0))
    fades = starts.sum(2)
    pos = torch.arange(n, device=win.device).expand_as(below_edge)
    last_out = torch.cummax(torch.where(below_edge, torch.full_like(pos, -1), pos), dim=2).values
    longest = torch.where(below_edge, pos - last_out, torch.zeros_like(pos)).amax(2)
    bins = torch.searchsorted((mean.unsqueeze(1) * g).contiguous(), p.contiguous(), right=True)
    hist = torch.zeros((B, g.numel() + 1), dtype=torch.int32, device=win.device).scatter_add_(1, bins, torch.ones_like(bins, dtype=torch.int32))
    x = p.unsqueeze(1) * (q.unsqueeze(0) / (mean.unsqueeze(1) * 2.0 ** 0.5)).unsqueeze(2)
    ber = 0.5 * torch.special.erfc(x).mean(2)
    return dict(mean=mean, mean_square=msq, minimum=win.amin(1), maximum=win.amax(1), below=below, fades=fades, longest_fade=longest, hist=hist, ber=ber)


res = {"mode": mode}
if mode == "calls":
    out_path = sys.argv[2]
    B, TH, Q = 1024, (-10.0, -6.0, -3.0), (6.0, 7.0)
    gen = torch.Generator("cuda").manual_seed(1)
    res["shape"] = dict(B=B, K=len(TH), E=32, Q=len(Q))
    for T in (1024, 4096):
        tels = [LinkTelemetry(B, length=T, device="cuda:0") for _ in range(2)]
        slow = torch.cumsum(0.05 * torch.randn((T + 17, B), device="cuda", generator=gen), 0)      # a random walk: fades last many frames
        power = (2e-4 * torch.exp(0.3 * torch.randn((T + 17, B), device="cuda", generator=gen) + slow - slow.mean(0))).float().contiguous()
        for k in range(T + 17):      # full and wrapped by 17 samples
            for t in tels:
                t.push(power[k])
        turn = [0]

        def stats():
            turn[0] ^= 1
            return tels[turn[0]].statistics(TH, "mean", None, Q)

        # the library call alone, into outputs made once
        i32, f32, f64 = torch.int32, torch.float32, torch.float64
        import ctypes as C
        from adaptive_optics_gym_amd.device_handle import ptr
        from adaptive_optics_gym_amd.link import default_hist_edges_db
        f, g, q = db_to_factor(TH), db_to_factor(default_hist_edges_db()), np.asarray(Q, dtype=np.float64)
        outs = [torch.empty(s, dtype=d, device="cuda") for s, d in (((B,), i32), ((B,), f64), ((B,), f64), ((B,), f32), ((B,), f32), ((B,), f64), ((B, 3), i32),
                                                                     ((B, 3), i32), ((B, 3), i32), ((B, 33), i32), ((B, 2), f64))]
        host = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

        def kernel():
            turn[0] ^= 1
            t = tels[turn[0]]
            t._call("statistics", 1, 0.0, host(f), 3, host(g), 32, host(q), 2, *[ptr(o) for o in outs], None, t._stream())

        win = torch.stack(tels[0].window())
        ft, gt, qt = (torch.as_tensor(a, device="cuda") for a in (f, g, q))
        got, want = tels[0].statistics(TH, "mean", None, Q), eager_statistics(win, ft, gt, qt)
        agree = {k: bool(torch.equal(got[k], want[k].to(got[k].dtype))) if not got[k].dtype.is_floating_point else float(((got[k] - want[k]).abs() / want[k].abs()).max())
                 for k in want}
        ring_bytes, out_bytes = 4 * T * B, sum(o.numel() * o.element_size() for o in outs)
        row = dict(kernel_us=timed(kernel), statistics_method_us=timed(stats), eager_torch_us=timed(lambda: eager_statistics(win, ft, gt, qt), calls=5, rounds=5, warm=2),
                   ring_bytes=ring_bytes, output_bytes=out_bytes, us_at_8TBps=(ring_bytes + out_bytes) / 8e6, eager_agrees=agree,
                   fade_fraction_3dB_mean=float(got["fade_fraction"][:, 2].mean()), fades_3dB_mean=float(got["fades"][:, 2].double().mean()))
        row["share_of_roof"] = row["us_at_8TBps"] / row["kernel_us"]["median"]
        res["T%d" % T] = row
        if T == 1024:
            res["push_us"] = timed(lambda: tels[0].push(power[5]), calls=200)
            res["push_bytes"] = 4 * B + 20 * B
        for t in tels:
            t.close()
elif mode == "rollout":
    label, out_path = sys.argv[3], sys.argv[4]
    B, N, A, T = 1024, 256, 64, 30
    env = BatchedAOEnv(B, "cuda:0", atm_type="quasi_static", atm_fried=0.20, act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T,
                       SH_operation=True, rew_type="strehl_ratio", seed=3, verbose=False)
    loops = {"ideal": lambda e: rollout(env, None, episodes=e, policy="ideal")}
    if LinkTelemetry is not None:
        tel = LinkTelemetry(B, length=1024, device=env.device)
        loops["ideal_link"] = lambda e: rollout(env, None, episodes=e, policy="ideal", link=tel)
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
    res["env_steps_per_s"] = {k: B / (float(np.median(v)) * 1e-6) for k, v in times.items()}
else:
    from adaptive_optics_gym_amd import ModalIntegrator

    out_path = sys.argv[2]
    B, N, A, T = 64, 64, 16, 1024
    res["closed_shape"] = dict(B=B, N=N, A=A, steps=T, atm_fried=0.1, atm_vel=10.0, window=1024, modal_gain=0.4)
    rows = {}
    for policy in ("ideal", "modal", "flat"):
        env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=10.0, atm_fried=0.1, act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T,
                           SH_operation=True, rew_type="strehl_ratio", seed=11, verbose=False)
        tel = LinkTelemetry(B, length=1024, device=env.device)
        if policy == "flat":
            env.reset()
            zero = torch.zeros((B, A), dtype=torch.float32, device=env.device)
            strehl = []
            for _ in range(T):
                r = env.step(zero)
                tel.push(r[4]["power"])
                strehl.append(r[4]["strehl"].clone())
            strehl = torch.stack(strehl)
        else:
            kw = dict(controller=ModalIntegrator(env, measurement="truth", gain=0.4)) if policy == "modal" else {}
            out = rollout(env, None, episodes=1, policy=policy, link=tel, **kw)
            strehl = (out["rew"].double() + 100.0) / 100.0
        rows[policy] = (tel, float(strehl.double().mean()))
    level = float(rows["ideal"][0].statistics()["mean"].mean())     # one absolute level for all three: the ideal controller's mean power
    for policy, (tel, strehl) in rows.items():
        row = {"mean_strehl": strehl}
        for name, reference in (("own_mean", "mean"), ("ideal_mean", level)):
            s = tel.statistics((-3.0,), reference, None, (6.0,))
            row[name] = dict(mean_power=float(s["mean"].mean()), scintillation_index=float(s["scintillation_index"].mean()),
                             fade_fraction_3dB=float(s["fade_fraction"].mean()), fades_3dB=float(s["fades"].double().mean()),
                             mean_fade_duration_3dB=float(torch.nanmean(s["mean_fade_duration"])), longest_fade_3dB=float(s["longest_fade"].double().mean()),
                             ber_q6=float(s["ber"].mean()))
        res[policy] = row
    res["ideal_mean_power"] = level
print(json.dumps(res))
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
