"""``get_state`` / ``set_state`` held to bit-identity for every stateful feature (checkpoint_harness.resume_case): a run interrupted after
k = 3 steps and resumed for m = 6 — in a fresh env built with the same arguments, and in the same env after it has moved on (and holds
whatever the feature leaves pending) — reproduces the uninterrupted run in every output, the final screens and the counters.  Episodes of
4 steps (3 where a snapshot needs an episode's end), so every resumed run crosses resets that draw from the restored streams.

Shapes: B = 5 (ragged against the env tiles of 32), N = 48 / 64, 6 / 8 Zernike modes or 16 actuators: the constructor spellings of each
feature's own test file.  The Shack-Hartmann cases need N = 128 (the pruned route with fused noise), B = 3.

A new stateful feature gets a case here; tests/test_checkpoint_fields_cpu.py reminds of the library's side."""
import numpy as np
import pytest

import checkpoint_harness as ch

pytestmark = pytest.mark.gpu

B, T, K, M = 5, 4, 3, 6


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _maker(check=None, cls=None, **kw):
    """``make()`` of a case: BatchedAOEnv(B, **kw) (``num_envs`` in kw: that many), the host tables computed once and shared."""
    _torch()
    shared = {}

    def make(**over):
        from adaptive_optics_gym_amd import BatchedAOEnv

        args = dict(kw, **over)
        n = args.pop("num_envs", B)
        env = (cls or BatchedAOEnv)(n, "cuda:0", verbose=False, **({"tables": shared["tables"]} if "tables" in shared and cls is None else {}), **args)
        shared.setdefault("tables", env.tables)
        if check is not None:
            check(env)
        return env
    return make


def _atm(atm, N=48, **more):
    """The existing checkpoint test's spelling (test_state_save_restore_resumes_bit_identically), per atmosphere type."""
    kw = dict(atm_type=atm, atm_vel=30 if atm == "dynamic" else 0, atm_fried=0.15, act_type="zernike", act_dim=8, obs_dim=2, num_pupil_pixels=N,
              timesteps_per_episode=T, seed=9, screen_source="device", screen_oversampling=4)
    kw.update(more)
    return kw


def _ring_direct(want):
    def check(env):
        assert env.info.reserved == want, "ring-direct" if want else "the repacking path"
    return check


# ---- 1 .. 4: the atmospheres x the step kernels, the other synthesis stream, the non-ring dynamic path -----------------------------------
PLAIN = {
    "quasi_static-mfma": (_atm("quasi_static", kernel="mfma"), None),
    "semi_dynamic-mfma": (_atm("semi_dynamic", kernel="mfma"), None),
    "dynamic-mfma-ring": (_atm("dynamic", kernel="mfma"), _ring_direct(1)),
    "quasi_static-valu": (_atm("quasi_static", kernel="valu"), None),
    "semi_dynamic-valu": (_atm("semi_dynamic", kernel="valu"), None),
    "dynamic-valu": (_atm("dynamic", kernel="valu"), _ring_direct(0)),
    "dynamic-fp64": (_atm("dynamic", precision="fp64"), None),
    "dynamic-f64-extrusion": (_atm("dynamic", extrusion="f64"), None),
    "semi_dynamic-hcipy16": (_atm("semi_dynamic", N=64, screen_method="hcipy16"), None),
}


@pytest.mark.parametrize("name", list(PLAIN))
def test_resume_plain_stepping(name):
    kw, check = PLAIN[name]
    n = ch.resume_case(_maker(check, **kw), ch.drive_with(T), K, M)
    assert n >= 6 * M + 2


def test_resume_dynamic_repacked(monkeypatch):
    """AOG_DYNAMIC_REPACK=1: the dynamic fast handle keeps psi_tile, psi_offset and psi_sum, and the blob carries them."""
    monkeypatch.setenv("AOG_DYNAMIC_REPACK", "1")
    ch.resume_case(_maker(_ring_direct(0), **_atm("dynamic", kernel="mfma")), ch.drive_with(T), K, M)


# ---- 5: lookahead, int8 and float64 extrusion: the restore lands on an extrusion launched ahead ----------------------------------------
@pytest.mark.parametrize("extrusion", ["auto", "f64"])
def test_resume_lookahead(extrusion):
    """Between two steps of a lookahead episode the screens stand at the next step and ``get_state`` refuses, so the episodes have 3 steps
    and the snapshot is taken at an episode's end.  The advanced env is reset and stepped once more first: its handle then holds the
    extrusion of the step after (``pre_evolved``; with the int8 form also what that prepared ahead), which the restore must drop."""
    from adaptive_optics_gym_amd import _lib

    def check(env):
        assert env.lookahead(True) is True
        assert (env.extrusion_kmax >= 1) == (extrusion == "auto")

    def leave_pending(env):
        env.reset()
        env.step(ch.actions_at(env))
        with pytest.raises(_lib.AogError, match="libaogym error -3"):
            env.get_state()

    make = _maker(check, **_atm("dynamic", N=64, atm_vel=30, extrusion=extrusion, timesteps_per_episode=3, act_type="num_actuators", act_dim=16))
    ch.resume_case(make, ch.drive_with(3), 3, M, before_restore=leave_pending)


def test_resume_restores_the_episode_position():
    """``steps_since_reset`` decides which step is an episode's last: that step launches no extrusion ahead (and queries no policy).  With
    lookahead switched on for the last step of every episode alone, a handle that knows its position launches nothing ahead, ever; one
    that resumed at the snapshot's step 3 of 4 with another position would launch the extrusion of a step that never comes, and the
    reset that follows would be refused."""
    def last_step_only(env):
        on = env.timestep % T == T - 1
        assert env.lookahead(on) is on
        return []

    ch.resume_case(_maker(**_atm("dynamic", N=64, act_type="num_actuators", act_dim=16)), ch.drive_with(T, before=last_step_only), K, M)


# ---- 6: pipelined stepping: the restore forgets the pending action -----------------------------------------------------------------------
def test_resume_pipelined():
    """``step(next_actions=...)`` as test_pipelined_stepping_is_bit_identical drives it, each drive ending its sequence (a snapshot needs
    that).  The advanced env is left with an action pending: after the restore the next step's action is not the announced one, and must
    be taken."""
    kw = dict(atm_type="dynamic", atm_vel=20.0, atm_fried=0.15, act_dim=16, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=64,
              timesteps_per_episode=T, seed=9, screen_oversampling=4)

    def nxt(env):
        a = np.random.RandomState(1000 + int(env.timestep) + 1).randn(env.num_envs, env.num_modes).astype(np.float32) * 0.5
        return _torch().from_numpy(a).to(env.device)

    def drive(env, n):
        out = []
        for i in range(n):
            rec = []
            if env.timestep % T == 0:
                obs, _ = env.reset()
                rec += [ch.cpu(obs), ch.cpu(env.last_obs_raw)]
            last = i == n - 1 or (env.timestep + 1) % T == 0
            ret = env.step(ch.actions_at(env), next_actions=None if last else nxt(env))
            out.append(rec + [ch.cpu(x) for x in ch.step_outputs(ret)])
        return out

    def leave_pending(env):
        assert env.timestep % T not in (0, T - 1)
        env.step(ch.actions_at(env), next_actions=nxt(env) * 2.0)
        with pytest.raises(RuntimeError):
            env.get_state()

    ch.resume_case(_maker(**kw), drive, K, M, before_restore=leave_pending)


# ---- 7: detector, per-env values ----------------------------------------------------------------------------------------------------------
def _det():
    return dict(obs_photons=np.exp(np.random.RandomState(5).uniform(np.log(5.0), np.log(5e4), B)), obs_read_noise=1.0, obs_background=0.5)


@pytest.mark.parametrize("atm", ["dynamic", "semi_dynamic"])
def test_resume_detector(atm):
    """The detector's frame counts resets as well as steps (``observation_frames``): both lie between the snapshot and the run's end."""
    kw = dict(atm_type=atm, atm_vel=20.0 if atm == "dynamic" else 0, act_dim=16, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=T, seed=21,
              screen_oversampling=4, **_det())
    ch.resume_case(_maker(**kw), ch.drive_with(T), K, M)


def test_resume_the_seed_travels_with_the_blob():
    """The blob's tail holds the handle's seed: on a static atmosphere, where nothing else depends on the constructor's seed, an env built
    with ANOTHER seed continues the saved screen-synthesis and detector streams."""
    kw = dict(atm_type="semi_dynamic", act_dim=16, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=T, seed=21, screen_oversampling=4, **_det())
    make = _maker(**kw)
    ch.resume_case(make, ch.drive_with(T), K, M, make_fresh=lambda: make(seed=22), halves=("fresh",))


# ---- 8: Shack-Hartmann with device noise on the pruned route -----------------------------------------------------------------------------
@pytest.mark.parametrize("three_pass", [False, True], ids=["separable", "three_pass"])
def test_resume_shack_hartmann_fused_noise(monkeypatch, three_pass):
    """N = 128: ``SH_step`` takes photon noise and lenslet sums inside the last propagation pass (the separable two-pass form, and with
    AOG_SH_THREE_PASS=1 the three-pass form, which keys the stream differently), counted by ``sh_calls``."""
    if three_pass:
        monkeypatch.setenv("AOG_SH_THREE_PASS", "1")
    kw = dict(atm_type="dynamic", atm_vel=30, atm_fried=0.15, act_type="zernike", act_dim=8, obs_dim=2, num_pupil_pixels=128, timesteps_per_episode=T,
              seed=4, screen_oversampling=4, SH_operation=True, num_envs=3)

    def sh_action(env):
        a, _ = env.SH_step()
        return a, [a]

    ch.resume_case(_maker(**kw), ch.drive_with(T, action=sh_action), K, M)


# ---- 9: set_turbulence with a mask before the snapshot ----------------------------------------------------------------------------------
def test_resume_after_set_turbulence():
    """r0 of some envs changes (and their screens are redrawn) in step 1; the fresh env is built with the constructor's values, so
    ``set_state`` hands the saved ones to the library itself (``_apply_fried``); the advanced env already runs at them."""
    old = np.array([(0.1, 0.2)[e % 2] for e in range(B)])
    mask = np.array([e % 3 == 0 for e in range(B)])
    kw = dict(atm_type="dynamic", atm_vel=8.0, atm_fried=old, act_type="num_actuators", act_dim=16, obs_dim=2, timesteps_per_episode=T,
              num_pupil_pixels=64, seed=3, screen_oversampling=4)

    def change(env):
        if env.timestep == 1:
            env.set_turbulence(0.15, mask)
        return [env.fried_parameters]

    def check(env):
        assert np.array_equal(env.fried_parameters, old)

    ch.resume_case(_maker(check, **kw), ch.drive_with(T, before=change), K, M)


# ---- 10: policy stepping with exploration noise ---------------------------------------------------------------------------------------------
class _PolicyRig:
    """An env with the policy and the OU process that explore it: one checkpoint of the three."""

    def __init__(self, env, policy, ou):
        self.env, self.policy, self.ou = env, policy, ou

    def __getattr__(self, name):
        return getattr(self.env, name)

    def get_state(self):
        return {"env": self.env.get_state(), "policy": self.policy.get_state(), "ou": self.ou.get_state()}

    def set_state(self, state):
        self.env.set_state(state["env"])
        self.policy.set_state(state["policy"])
        self.ou.set_state(state["ou"])


def test_resume_policy_stepping_with_exploration_noise():
    """``reset_with_policy`` / ``step_with_policy`` with dropout, Gaussian and Ornstein-Uhlenbeck noise (test_gpu_action_noise.py's
    spelling; 16 units: one output tile, so log_prob is bit-exact).  The streams are keyed by the policy's call index and the OU state,
    which are the policy's and the process's to save (``DeviceActor.get_state``, ``DeviceOUNoise.get_state``): the env's state does not
    and cannot hold them.  A policy-attached step leaves an action pending until the episode's last step, so the episodes have 3 steps
    and the snapshot is taken at an episode's end; the advanced env is reset with the policy first, which leaves one pending."""
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor, DeviceOUNoise, make_actor

    Te, A = 3, 16
    torch.manual_seed(5)
    actor = make_actor(4, A, 150, device="cuda:0")
    with torch.no_grad():
        actor.out.weight.mul_(100.0)
    make_env = _maker(atm_type="dynamic", atm_vel=20.0, act_dim=A, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=Te, seed=4, screen_oversampling=4)

    def make():
        return _PolicyRig(make_env(), DeviceActor(actor, seed=11), DeviceOUNoise(B, A, 0.0, 0.3, 0.05, device="cuda:0"))

    def drive(rig, n):
        out = []
        for _ in range(n):
            rec = []
            if rig.timestep % Te == 0:
                (obs, _), pol = rig.env.reset_with_policy(rig.policy, ou_noise=rig.ou)
                rec += [ch.cpu(x) for x in (obs, rig.env.last_obs_raw, *pol)]
            ret, pol = rig.env.step_with_policy(rig.policy, ou_noise=rig.ou)
            assert (pol is None) == (rig.timestep % Te == 0)
            rec += [ch.cpu(x) for x in ch.step_outputs(ret) + (list(pol) if pol is not None else []) + [rig.ou.state]]
            rec.append(np.array(rig.policy.calls))
            out.append(rec)
        return out

    def leave_pending(rig):
        rig.env.reset_with_policy(rig.policy, ou_noise=rig.ou)
        with pytest.raises(RuntimeError):
            rig.env.get_state()

    n = ch.resume_case(make, drive, 3, M, before_restore=leave_pending)
    assert n == M * 8 + 2 * 5 + 4 * 3   # (every step 6 outputs, the OU state and the call index; 2 resets; 4 queries by a step)


# ---- 11: pyramid sensor with photon noise -------------------------------------------------------------------------------------------------
PYR = dict(samples=16, pixels=16, n_mod=2, r_mod=1.0)   # (test_photon_noise_follows_the_reference_stream's sensor)


def _pyramid_kw(photons):
    return dict(atm_type="semi_dynamic", act_type="zernike", act_dim=6, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=64, timesteps_per_episode=T,
                seed=77, screen_oversampling=4, pyramid=dict(PYR, photons=photons))


def _sense(env):
    """Frames, slopes and the integrator's update: three sensor calls, three frames of the photon stream."""
    frames, slopes = env.pyramid_frames(), env.pyramid_slopes()
    act, s = env.PYR_step()
    assert not bool((slopes == s).all()), "two sensor calls drew the same photons"
    return [frames, slopes, act, s]


@pytest.mark.parametrize("photons", [400.0, 3.0], ids=["normal_branch", "inversion_branch"])
def test_resume_pyramid_photon_noise(photons):
    """The sensor's photon stream is keyed by its call count, which is saved and restored (``pyramid_frame_count``, the blob's tail)."""
    ch.resume_case(_maker(**_pyramid_kw(photons)), ch.drive_with(T, before=_sense), K, M)


def test_resume_pyramid_uploaded_by_the_restore():
    """A fresh env whose sensor is not on the handle yet when the state arrives: the upload restarts the library's count, so it has to come
    before the restore (``set_state`` sees to it), not with the first sensor call after it."""
    make = _maker(**_pyramid_kw(400.0))

    def make_fresh():
        env = make()
        env._pyramid_uploaded = False   # (as if nothing had uploaded the sensor so far: whoever needs it first uploads it)
        return env

    ch.resume_case(make, ch.drive_with(T, before=_sense), K, M, make_fresh=make_fresh, halves=("fresh",))


# ---- 12: the science camera is NOT state ---------------------------------------------------------------------------------------------------
def test_resume_beside_the_science_camera():
    """The exposure is measurement data: ``set_state`` leaves it bit for bit as it was (read immediately before and after, on the advanced
    env with 6 frames in it), and the frames integrated after the restore are those of the uninterrupted run once each camera was cleared
    at the snapshot point."""
    kw = dict(atm_type="dynamic", atm_vel=20.0, atm_fried=0.15, act_dim=16, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=64,
              timesteps_per_episode=T, seed=9, screen_oversampling=4, science_window=48)
    keys = ("psf", "strehl", "encircled_energy", "frames")

    def read(env):
        exp = env.science_exposure()
        return [ch.cpu(exp[k]) for k in keys]

    def integrate(env):
        env.science_integrate()
        return read(env)

    def restore(env, snap):
        before = read(env)
        assert (before[3] == M).all() and before[0].max() > 0
        env.set_state(snap)
        for k, x, y in zip(keys, before, read(env)):
            np.testing.assert_array_equal(y, x, err_msg=f"set_state changed the science camera's {k}")

    ch.resume_case(_maker(**kw), ch.drive_with(T, after=integrate), K, M, at_snapshot=lambda env: env.science_clear(), restore=restore)


# ---- 13: layered atmosphere, the advanced half ---------------------------------------------------------------------------------------------
def test_resume_layered_advanced():
    """Two layers through ``LayeredAOEnv``'s own ``get_state`` / ``set_state``, restored into the env itself after 6 further steps (the
    fresh half is test_gpu_layered.py's)."""
    from adaptive_optics_gym_amd import LayeredAOEnv

    kw = dict(atm_layers=[{"fraction": 0.6, "speed": 30.0}, {"fraction": 0.4, "speed": 50.0}], atm_fried=0.15, seed=11, act_type="zernike", act_dim=6,
              obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=T, num_pupil_pixels=32)

    def layers(env):
        return [env.layer_screens(l) for l in range(env.num_layers)]

    ch.resume_case(_maker(cls=LayeredAOEnv, **kw), ch.drive_with(T, after=layers), K, M, halves=("advanced",))


# ---- states of another configuration are refused --------------------------------------------------------------------------------------------
def test_mismatched_states_are_refused():
    base = dict(act_type="zernike", act_dim=6, obs_dim=2, num_pupil_pixels=64, timesteps_per_episode=T, seed=77, screen_oversampling=4)
    make = _maker(**base)
    envs = dict(plain=make(), small=make(num_envs=2), det=make(obs_photons=1e3, obs_read_noise=1.0), pyr=make(pyramid=dict(PYR, photons=400.0)))
    try:
        states = {k: e.get_state() for k, e in envs.items()}
        # (B = 5 and B = 2 share one env tile, and every part of the blob is padded to 256 bytes: the two blobs have ONE size, so the blob
        # alone does not tell them apart; the refusal must come before the handle is written)
        assert states["small"]["blob"].numel() == states["plain"]["blob"].numel()
        screens = envs["small"].get_screens().clone()
        with pytest.raises(ValueError, match="saved with num_envs = 5 and this environment has 2"):
            envs["small"].set_state(states["plain"])
        assert _torch().equal(envs["small"].get_screens(), screens), "a refused state was written into the handle"
        with pytest.raises(ValueError, match="state blob does not match this environment's configuration"):
            envs["small"].set_state(dict(states["small"], blob=states["small"]["blob"][:-256]))
        with pytest.raises(ValueError, match="saved without a detector and this environment was built with one"):
            envs["det"].set_state(states["plain"])
        with pytest.raises(ValueError, match="saved with a detector and this environment was built without one"):
            envs["plain"].set_state(states["det"])
        with pytest.raises(ValueError, match="saved with a pyramid sensor and this environment was built without one"):
            envs["plain"].set_state(states["pyr"])
        with pytest.raises(ValueError, match="saved without a pyramid sensor and this environment was built with one"):
            envs["pyr"].set_state(states["plain"])
        for k, e in envs.items():   # a refusal changed nothing: each still takes its own state
            e.set_state(states[k])
            assert e.device_status() == 0
    finally:
        for e in envs.values():
            e.close()
