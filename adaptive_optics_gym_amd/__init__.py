"""MI355X-native implementation of the AOEnv.reset()/step() hot path of payamparvizi/adaptive_optics_gym.

    from adaptive_optics_gym_amd import BatchedAOEnv      # B envs on one GPU, torch tensors
    from adaptive_optics_gym_amd import LayeredAOEnv      # the same over several frozen-flow wind layers per env
    from adaptive_optics_gym_amd.envs import AOEnv        # the reference's single-env gym API
    from adaptive_optics_gym_amd import ModalTelemetry, ModalIntegrator   # loop telemetry (PSDs) and the optimised modal integrator
    from adaptive_optics_gym_amd import LQGController     # the LQG baseline: per-mode Kalman prediction of turbulence and vibration lines
    from adaptive_optics_gym_amd import LinkTelemetry     # the optical link's read-out: fades, power histogram, bit-error rate
    from adaptive_optics_gym_amd import ModalDisturbance  # vibration and static aberrations for LayeredAOEnv(disturbance=...)
    from adaptive_optics_gym_amd import MirrorServo       # loop latency and mirror dynamics for BatchedAOEnv(servo=...)
    from adaptive_optics_gym_amd.tomography import TomographicController   # the MCAO baseline of LayeredAOEnv(altitude_mirrors=...)
    from adaptive_optics_gym_amd.scintillation import rytov_variance       # the regime check of LayeredAOEnv(scintillation=...)
    import gym_AO                                         # registers 'AO-v0' like the reference (needs gymnasium)
"""
from .batched_env import BatchedAOEnv  # noqa: F401
from .disturbance import ModalDisturbance  # noqa: F401
from .layered import LayeredAOEnv, Sightline  # noqa: F401
from .link import LinkTelemetry  # noqa: F401
from .lqg import LQGController  # noqa: F401
from .params import OpticalParams  # noqa: F401
from .servo import MirrorServo  # noqa: F401
from .telemetry import ModalIntegrator, ModalTelemetry  # noqa: F401

__all__ = ["BatchedAOEnv", "LQGController", "LayeredAOEnv", "LinkTelemetry", "MirrorServo", "ModalDisturbance", "ModalIntegrator", "ModalTelemetry", "OpticalParams", "Sightline", "register"]


def register():
    """gym_AO/__init__.py:9-12 — register 'AO-v0' with gymnasium when it is importable."""
    try:
        from gymnasium.envs.registration import register as _register, registry
    except Exception:
        return False
    if "AO-v0" not in registry:
        _register(id="AO-v0", entry_point="adaptive_optics_gym_amd.envs:AOEnv")
    return True
