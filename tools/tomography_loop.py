"""The closed loop of profiles/tomography.md: Strehl and mean power on an uplink sightline for a flat mirror, 'ideal' on the beacon and
the tomographic controller with the beacon and the uplink as guide directions, and the cost of a step of each loop.
``python tools/tomography_loop.py [num_envs] [N] [steps] [seed]``."""
import sys
import time

import numpy as np
import torch

from adaptive_optics_gym_amd import LayeredAOEnv
from adaptive_optics_gym_amd.tomography import TomographicController


def main():
    B, N, T, seed = (int(x) for x in (sys.argv[1:5] + ["64", "64", "200", "7"][len(sys.argv) - 1:]))
    uplink = (6e-6, 0.0)      # 6 urad: 0.06 m = 7.7 pixels at 10 km

    def make():
        return LayeredAOEnv(B, "cuda:0", atm_layers=[{"fraction": 0.6, "speed": 8.0}, {"fraction": 0.4, "speed": 25.0}], atm_fried=0.1, seed=seed,
                            act_type="zernike", act_dim=20, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=T, SH_operation=True, verbose=False,
                            layer_altitudes=[0.0, 1e4], altitude_mirrors=[dict(altitude=1e4, actuators=9)], sightlines={"uplink": uplink})

    print(f"B={B} N={N} steps={T} seed={seed} r0=0.1 m, layers at 0 and 10 km (0.6 / 0.4), uplink {uplink} rad, 20 Zernike modes + one 9x9 mirror at 10 km")
    for name in ("flat", "ideal", "tomographic"):
        env = make()
        ctrl = TomographicController(env, guide_stars=("self", "uplink"), gain=0.5) if name == "tomographic" else None
        env.reset()
        zero = torch.zeros((B, env.num_modes), dtype=torch.float32, device="cuda")
        up_s, up_p, own_s = [], [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            a = zero if name == "flat" else (env.ideal_action() if name == "ideal" else ctrl.action()).to(torch.float32)
            info = env.step(a)[4]
            if t >= T // 4:      # (the loop has closed)
                up_s.append(info["sightlines"]["uplink"]["strehl"]), up_p.append(info["sightlines"]["uplink"]["power"]), own_s.append(info["strehl"])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / T
        mean = lambda xs: float(torch.stack(xs).double().mean())
        print(f"{name:12s} uplink Strehl {mean(up_s):.4f}  uplink mean power {mean(up_p):.5g}  beacon Strehl {mean(own_s):.4f}   {dt * 1e6:.0f} us per step (host wall)")
        if ctrl is not None:
            ctrl.close()
        env.close()


if __name__ == "__main__":
    main()
