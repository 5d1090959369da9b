"""The science camera on the device (aog_upload_science / aog_science_integrate / aog_science_clear / aog_science_read): frames against the
oracle's science-arm image, exposures as sums of frames, independence of how envs are grouped, encircled energy, and the step path left
alone."""
import numpy as np
import pytest

from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

RTOL = 1e-5
# (N, B, act_type, A, window, precision): partial env tiles and a ragged 240 inside 256; N no multiple of 32 or 128; a window that is no
# multiple of 32; the float64 validation form; five 32-column blocks (pass 1's second workgroup has three waves without a block, pass 2's
# second workgroup row one block)
SHAPES = [(64, 37, "num_actuators", 16, 240, "fast"), (240, 3, "num_actuators", 64, 64, "fast"), (128, 5, "zernike", 6, 48, "fast"),
          (64, 2, "num_actuators", 16, 240, "fp64"), (64, 3, "num_actuators", 16, 160, "fast")]


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _image_error(power, ref_power):
    """The project's image rule (_assert_power_image_close of test_gpu_parity.py): 1e-5 relative per pixel, pixels below 1e-3 of the image's
    peak held to the same ABSOLUTE error (1e-8 x peak).  Returns the worst error in units of that tolerance."""
    tol = RTOL * np.maximum(ref_power, 1e-3 * ref_power.max())
    return float(np.max(np.abs(power - ref_power) / tol))


_FRAMES = {}


def _one_frame(shape):
    """reset, one step, clear, integrate, read on the device, and the oracle's science image of the sampled envs; computed once per shape."""
    if shape in _FRAMES:
        return _FRAMES[shape]
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv
    from oracle.ao_env_oracle import AOEnvOracle

    N, B, act_type, A, w, precision = shape
    scr = smooth_screens(B, N, 40 + N)
    a = actions_for(B, A, 6)
    kw = dict(act_type=act_type, act_dim=A, obs_dim=2, rew_type="strehl_ratio", timesteps_per_episode=5)
    env = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, screens=scr, precision=precision, science_window=w, verbose=False, **kw)
    env.reset()
    _, _, _, _, info = env.step(torch.from_numpy(a).cuda())
    env.science_clear()
    env.science_integrate()
    got = {k: v.cpu().numpy() for k, v in env.science_exposure().items()}
    got["step_strehl"] = info["strehl"].cpu().numpy().astype(np.float64)
    got["radii"] = env.science_radii
    env.close()
    refs = {}
    for b in sorted({0, B // 2, B - 1}):
        ref = AOEnvOracle(num_pupil_pixels=N, screen=scr[b].ravel(), verbose=False, **kw)
        ref.reset()
        ref.step(a[b])
        total = ref.wf_wfs.total_power
        power = ref.wf_sci_focal_plane.power.reshape(240, 240)
        refs[b] = dict(image=power / (ref.unaberrated_PSF.max() * total), share=power / total,
                       r=np.hypot(ref.focal_grid.x, ref.focal_grid.y).reshape(240, 240) / (ref.wavelength_sci / ref.telescope_diameter))
    _FRAMES[shape] = got, refs
    return _FRAMES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-B%d-%s%d-w%d-%s" % s)
def test_one_frame_matches_the_oracle_image(shape):
    got, refs = _one_frame(shape)
    N, B, _, _, w, _ = shape
    assert got["psf"].shape == (B, w, w) and got["psf"].dtype == np.float64 and (got["frames"] == 1).all()
    lo = 120 - w // 2
    worst = max(_image_error(got["psf"][b], r["image"][lo:lo + w, lo:lo + w]) for b, r in refs.items())
    print(f"science camera, one frame, shape {shape}: worst error {worst:.3f} x tolerance")
    assert worst <= 1.0, f"worst {worst:.2f} x tol"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-B%d-%s%d-w%d-%s" % s)
def test_centre_pixel_is_the_steps_strehl(shape):
    got, _ = _one_frame(shape)
    w = shape[4]
    np.testing.assert_array_equal(got["strehl"], got["psf"][:, w // 2, w // 2])
    np.testing.assert_allclose(got["strehl"], got["step_strehl"], rtol=RTOL)


def test_encircled_energy_matches_the_oracle_and_is_monotone():
    for shape in SHAPES:
        got, refs = _one_frame(shape)
        ee = got["encircled_energy"]
        assert ee.shape == (shape[1], len(got["radii"])) and (np.diff(ee, axis=1) >= 0).all() and (ee <= 1).all() and (ee > 0).all()
        if shape[4] != 240:
            continue
        np.testing.assert_array_equal(got["radii"], [1, 2, 3, 5, 8])
        for b, r in refs.items():
            want = [r["share"][r["r"] <= R * (1 + 1e-9)].sum() for R in got["radii"]]
            np.testing.assert_allclose(ee[b], want, rtol=RTOL)


DYN = dict(atm_type="dynamic", atm_vel=20.0, atm_fried=0.15, act_dim=16, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=64,
           timesteps_per_episode=6, seed=9, screen_oversampling=4, verbose=False)


def test_exposure_is_the_sum_of_its_frames_and_masks_select_envs():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, T = 70, 6
    acts = torch.from_numpy(np.random.RandomState(3).randn(T, B, 16).astype(np.float32)).cuda()
    env, twin = (BatchedAOEnv(B, "cuda:0", science_window=64, **DYN) for _ in range(2))
    env.reset()
    twin.reset()
    frames = []
    for t in range(T):
        env.step(acts[t])
        twin.step(acts[t])
        env.science_integrate()
        twin.science_clear()
        twin.science_integrate()
        one = twin.science_exposure()
        assert (one["frames"] == 1).all()
        frames.append(one["psf"].clone())
    exp = env.science_exposure()
    assert (exp["frames"] == T).all() and exp["frames"].dtype == torch.int32
    assert not torch.equal(frames[0], frames[-1])   # (the wind moved the screens)
    mean = torch.stack(frames).sum(0) / T
    torch.testing.assert_close(exp["psf"], mean, rtol=1e-13, atol=0)
    torch.testing.assert_close(exp["strehl"], mean[:, 32, 32], rtol=1e-13, atol=0)
    # a masked integrate and a masked clear touch the selected envs alone
    sel = [1, 33, 69]
    mask = np.zeros(B, dtype=bool)
    mask[sel] = True
    before = env.science_exposure()
    env.science_integrate(mask=mask)
    after = env.science_exposure()
    rest = torch.from_numpy(~mask).cuda()
    assert (after["frames"][sel] == T + 1).all() and (after["frames"][rest] == T).all()
    for k in ("psf", "strehl", "encircled_energy"):
        assert torch.equal(after[k][rest], before[k][rest])
        assert all(not torch.equal(after[k][i], before[k][i]) for i in sel)
    env.science_clear(mask=torch.from_numpy(mask))
    cleared = env.science_exposure()
    assert (cleared["frames"][sel] == 0).all() and (cleared["frames"][rest] == T).all()
    assert float(cleared["psf"][sel].abs().max()) == 0 and torch.equal(cleared["psf"][rest], before["psf"][rest])
    env.close()
    twin.close()


def test_grouping_of_envs_does_not_matter(monkeypatch):
    """Two handles of 35 with their env_id_base, chunks of 32 envs, one integrate through two complementary masks, and the other tile
    geometry each give the plain run's psf, Strehl and encircled energy bit for bit."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, N, A = 70, 64, 16
    scr = smooth_screens(B, N, 21)
    a = torch.from_numpy(actions_for(B, A, 8)).cuda()
    kw = dict(act_dim=A, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=N, timesteps_per_episode=5, science_window=64, verbose=False)

    def run(n, offset, integrate, chunk=None):
        if chunk:
            monkeypatch.setenv("AOG_SCIENCE_CHUNK", str(chunk))
        else:
            monkeypatch.delenv("AOG_SCIENCE_CHUNK", raising=False)
        env = BatchedAOEnv(n, "cuda:0", screens=scr[offset:offset + n], global_env_offset=offset, total_envs=B, pixel_chunks=8, **kw)
        env.reset()
        env.step(a[offset:offset + n])
        integrate(env)
        out = {k: v.clone() for k, v in env.science_exposure().items()}
        env.close()
        return out

    def two_masks(env):
        m = np.arange(B) % 3 == 0
        m[40:] = ~m[40:]
        env.science_integrate(mask=m)
        env.science_integrate(mask=~m)

    plain = run(B, 0, lambda e: e.science_integrate())
    assert float(plain["strehl"].min()) > 0 and (plain["frames"] == 1).all()
    halves = [run(35, off, lambda e: e.science_integrate()) for off in (0, 35)]
    variants = {"halves": {k: torch.cat([h[k] for h in halves]) for k in plain}, "chunked": run(B, 0, lambda e: e.science_integrate(), chunk=32),
                "masks": run(B, 0, two_masks)}
    # the two tile geometries of a window of two blocks (four waves sharing the blocks, or one block per wave with idle waves)
    monkeypatch.setenv("AOG_SCIENCE_SPLIT", "0")
    variants["one block per wave"] = run(B, 0, lambda e: e.science_integrate())
    monkeypatch.delenv("AOG_SCIENCE_SPLIT")
    for name, got in variants.items():
        for k in ("psf", "strehl", "encircled_energy", "frames"):
            assert torch.equal(got[k], plain[k]), (name, k)


@pytest.mark.parametrize("atm", ["quasi_static", "dynamic"])
def test_the_step_path_is_untouched(atm):
    """A handle that integrates after every step of two episodes returns what a handle without the camera returns, bit for bit."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    B, T = 70, 6
    kw = dict(DYN, atm_type=atm, atm_vel=20.0 if atm == "dynamic" else 0)
    acts = torch.from_numpy(np.random.RandomState(5).randn(2 * T, B, 16).astype(np.float32)).cuda()

    def run(camera):
        env = BatchedAOEnv(B, "cuda:0", science_window=64 if camera else None, **kw)
        outs = []
        for ep in range(2):
            obs0, _ = env.reset()
            outs.append(obs0.clone())
            for t in range(T):
                r = env.step(acts[ep * T + t])
                outs.extend([r[0].clone(), r[1].clone(), r[2].clone(), r[4]["obs_raw"].clone(), r[4]["power"].clone(), r[4]["strehl"].clone()])
                if camera:
                    env.science_integrate()
        if camera:
            assert (env.science_exposure(image=False)["frames"] == 2 * T).all()
        outs.append(env.get_actuators().clone())
        env.close()
        return outs

    plain, cam = run(False), run(True)
    assert len(plain) == len(cam)
    for x, y in zip(plain, cam):
        assert torch.equal(x, y)


def test_camera_is_refused_while_the_next_step_is_already_in_place():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, _lib

    B, T = 40, 6
    acts = torch.from_numpy(np.random.RandomState(6).randn(T, B, 16).astype(np.float32)).cuda()
    env = BatchedAOEnv(B, "cuda:0", science_window=48, **dict(DYN, atm_type="quasi_static", atm_vel=0))
    env.reset()
    env.step(acts[0], next_actions=acts[1])   # mid-sequence: the mirror already belongs to the next step
    for call in (env.science_integrate, env.science_clear, env.science_exposure):
        with pytest.raises(RuntimeError, match="libaogym error -3"):
            call()
    env.step(acts[1], next_actions=None)   # ends the sequence
    env.science_integrate()
    assert (env.science_exposure(image=False)["frames"] == 1).all()
    env.close()
    env = BatchedAOEnv(B, "cuda:0", science_window=48, **DYN)
    assert env.lookahead(True)
    env.reset()
    env.step(acts[0])
    with pytest.raises(_lib.AogError, match="libaogym error -3"):   # between two lookahead steps the screens stand at the next one
        env.science_integrate()
    for t in range(1, T):
        env.step(acts[t])
    env.science_integrate()   # episode boundary: allowed
    assert (env.science_exposure(image=False)["frames"] == 1).all()
    env.close()


def test_refusals_and_bookkeeping():
    torch = _torch()
    import ctypes as C

    from adaptive_optics_gym_amd import BatchedAOEnv, _lib
    from adaptive_optics_gym_amd.rollout import make_actor, rollout

    B, N, A = 5, 64, 16
    kw = dict(act_dim=A, obs_dim=2, rew_type="strehl_ratio", num_pupil_pixels=N, timesteps_per_episode=3, screens=smooth_screens(B, N, 2), verbose=False)
    for bad in (63, 0, 242):
        with pytest.raises(ValueError, match="science_window"):
            BatchedAOEnv(B, "cuda:0", science_window=bad, **kw)
    with pytest.raises(ValueError, match="science_radii"):
        BatchedAOEnv(B, "cuda:0", science_radii=[1.0], **kw)
    plain = BatchedAOEnv(B, "cuda:0", **kw)
    # a handle without the camera: Python refuses, the library refuses (before the upload), and nothing was allocated for it
    for call in (plain.science_integrate, plain.science_clear, plain.science_exposure):
        with pytest.raises(ValueError, match="science camera"):
            call()
    assert plain.lib.aog_science_integrate(plain._handle, None, None) == -3 and b"not uploaded" in plain.lib.aog_last_error()
    assert plain.lib.aog_science_read(plain._handle, 0, 1, None, None, None, None, None) == -1
    with pytest.raises(ValueError, match="science_window"):
        rollout(plain, None, science=True)
    cam = BatchedAOEnv(B, "cuda:0", science_window=48, science_radii=[1.0, 2.5], **kw)
    assert cam.science_window == 48 and cam.science_radii.tolist() == [1.0, 2.5]
    base = plain.device_bytes()
    w2 = 48 * 48
    assert cam.device_bytes() > base + B * w2 * 8
    # the library's own checks of a window (a caller that bypasses Python)
    m = np.zeros((48, N, 2))
    bins = np.zeros(w2, dtype=np.int32)
    p = lambda arr: C.c_void_p(arr.ctypes.data)
    for w_bad in (47, 0):
        assert cam.lib.aog_upload_science(cam._handle, p(m), p(m), w_bad, 0.68, 0.05, p(bins), 1) == -1
    # zero frames read as zeros; counts and the range check
    cam.reset()
    z = cam.science_exposure()
    assert all(float(z[k].abs().max()) == 0 for k in ("psf", "strehl", "encircled_energy")) and (z["frames"] == 0).all()
    for first, count in ((3, 3), (-1, 2), (0, -1), (6, None)):
        with pytest.raises(ValueError, match="science_exposure"):
            cam.science_exposure(first=first, count=count)
    assert cam.lib.aog_science_read(cam._handle, 3, 3, None, C.c_void_p(z["strehl"].data_ptr()), None, None, None) == -1   # (the library's own range check)
    with pytest.raises(ValueError, match="mask"):
        cam.science_integrate(mask=np.ones(B + 1, dtype=bool))
    # rollout(science=True) integrates after every step and never clears
    torch.manual_seed(12)
    rollout(cam, make_actor(4, A, 32, device="cuda:0"), episodes=2, science=True)
    out = cam.science_exposure(1, 3, image=False)
    assert (out["frames"] == 6).all() and "psf" not in out and out["encircled_energy"].shape == (3, 2) and float(out["strehl"].min()) > 0
    assert plain.device_bytes() == base
    plain.close()
    # what a handle without the camera owned before the camera existed, measured on the parent commit for this construction: the camera's
    # buffers are allocated by aog_upload_science alone
    old = BatchedAOEnv(5, "cuda:0", num_pupil_pixels=64, act_dim=16, obs_dim=2, rew_type="strehl_ratio", seed=3, verbose=False)
    assert old.device_bytes() == 4482528
    old.close()
    cam.close()
