"""The closed-loop figure of profiles/telemetry.md: a small dynamic env, the pyramid sensor with photon noise, ModalIntegrator at the
uniform default gain against the same loop after retune(), over the same seeds.  Both loops run WARM steps at the default gain (the
retuned one records its telemetry there), then STEPS steps whose residual error energy sum rms^2 (wavefront_truth, after every step) is
compared.  One JSON line."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from adaptive_optics_gym_amd import BatchedAOEnv, ModalIntegrator, ModalTelemetry

B, A, WARM, STEPS, PHOTONS = 8, 16, 256, 256, float(os.environ.get("PHOTONS", "2000"))
res = {}
for seed in (3, 4, 5):
    for retune in (False, True):
        env = BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=20.0, SH_operation=True, act_dim=A, obs_dim=2, num_pupil_pixels=32,
                           timesteps_per_episode=WARM + STEPS + 1, seed=seed, verbose=False,
                           pyramid=dict(samples=16, pixels=16, n_mod=4, r_mod=2.0, photons=PHOTONS))
        ctrl = ModalIntegrator(env, measurement="pyramid", delay=1, gain=0.4, telemetry=ModalTelemetry(B, A, length=256, device=env.device))
        env.reset()
        energy = torch.zeros(B, dtype=torch.float64, device="cuda")
        fit = torch.zeros(B, dtype=torch.float64, device="cuda")
        for t in range(WARM + STEPS):
            if t == WARM and retune:
                ctrl.retune(segment=64)
            env.step(ctrl.action().float())
            if t >= WARM:
                w = env.wavefront_truth()
                energy += w["rms"] ** 2
                fit += w["fit_rms"] ** 2
        key = "retuned" if retune else "uniform"
        res.setdefault(key, []).append(float(energy.sum()))
        res.setdefault(key + "_fit", []).append(float(fit.sum()))
        if retune:
            res.setdefault("gains_min_median_max", []).append([float(ctrl.gains.min()), float(ctrl.gains.median()), float(ctrl.gains.max())])
        ctrl.close()
        env.close()
res["ratio_retuned_over_uniform"] = [r / u for r, u in zip(res["retuned"], res["uniform"])]
res["ratio_all_seeds"] = sum(res["retuned"]) / sum(res["uniform"])
res["photons"] = PHOTONS
print(json.dumps(res))
