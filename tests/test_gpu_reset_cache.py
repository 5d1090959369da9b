"""The reset observation kept between episodes (aog_env::reset_obs_valid, k_reset_cached): a handle whose screens stay, with a flat mirror
start, the table route and no detector answers every reset after the first from a copy of that first observation, in one launch.  Every test
drives such a handle and a twin built under AOG_RESET_CACHE=0 (every reset runs the pupil pass, as before the cache existed) in the same way
and compares them bit for bit.  N = 64, B = 96 (three env tiles, not a multiple of 64), A = 16."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from helpers import actions_for, smooth_screens

pytestmark = pytest.mark.gpu

N, B, A = 64, 96, 16
MASKED = [0, 31, 32, 95]
_TABLES = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(**kw):
    from adaptive_optics_gym_amd import BatchedAOEnv

    base = dict(act_dim=A, obs_dim=2, num_pupil_pixels=N, timesteps_per_episode=3, seed=21, screen_oversampling=4, verbose=False)
    base.update(kw)
    key = (base["obs_dim"], base["act_dim"], base.get("precision", "fast"))
    env = BatchedAOEnv(B, "cuda:0", tables=_TABLES.get(key), **base)   # (the host tables are computed once per shape)
    _TABLES.setdefault(key, env.tables)
    return env


@pytest.fixture
def pair(monkeypatch):
    """pair(**kw) -> (handle with the cache, twin without); closed at the end of the test."""
    made = []

    def make(**kw):
        monkeypatch.delenv("AOG_RESET_CACHE", raising=False)
        env = _env(**kw)
        made.append(env)
        monkeypatch.setenv("AOG_RESET_CACHE", "0")
        twin = _env(**kw)
        made.append(twin)
        monkeypatch.delenv("AOG_RESET_CACHE")
        return env, twin

    yield make
    for e in made:
        e.close()


def _actions(seed):
    return _torch().from_numpy(actions_for(B, A, seed)).cuda()


def _same_reset(env, twin, mask=None):
    """reset both; the observations must agree bit for bit.  Returns the cached handle's (obs, obs_raw) clones."""
    torch = _torch()
    o1, _ = env.reset(mask=mask)
    o2, _ = twin.reset(mask=mask)
    assert torch.equal(o1, o2) and torch.equal(env.last_obs_raw, twin.last_obs_raw)
    return o1.clone(), env.last_obs_raw.clone()


def _same_steps(env, twin, seeds):
    torch = _torch()
    for s in seeds:
        a = _actions(s)
        r1, r2 = env.step(a), twin.step(a)
        for k in (0, 1, 2):
            assert torch.equal(r1[k], r2[k]), f"step (seed {s}) output {k}"
        for k in ("obs_raw", "power", "strehl"):
            assert torch.equal(r1[4][k], r2[4][k]), f"step (seed {s}) {k}"


def _blob(env):
    """The library's state blob (actuators, t_render, screens, counters) in a zeroed buffer: the padding between its parts is not written."""
    torch = _torch()
    blob = torch.zeros((int(env.lib.aog_state_bytes(env._handle)),), dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert env.lib.aog_get_state(env._handle, C.c_void_p(blob.data_ptr()), None, stream) == 0
    return blob


def _fused_launches(env):
    return env.profile_read()[1]


# ---- 1. hit == miss ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(obs_dim=2), dict(obs_dim=5, rew_type="smf_ssim")], ids=["o2_strehl", "o5_ssim_mrw28"])
def test_cached_reset_equals_the_pupil_pass(pair, kw):
    torch = _torch()
    env, twin = pair(**kw)
    first = _same_reset(env, twin)                 # fills
    _same_steps(env, twin, (1, 2, 3))
    again = _same_reset(env, twin)                 # hits
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(env.get_actuators(), twin.get_actuators()) and float(env.get_actuators().abs().max()) == 0
    assert torch.equal(_blob(env), _blob(twin))
    _same_steps(env, twin, (4, 5, 6))
    _same_reset(env, twin)
    assert env.device_status() == 0 and twin.device_status() == 0


# ---- 2. the hit skips the pass -----------------------------------------------------------------------------------------------------------------
def test_cached_reset_launches_no_pupil_pass(pair):
    env, twin = pair()
    for e in (env, twin):
        e.profile(True, every=1, block=1)
    env.reset()
    twin.reset()
    assert _fused_launches(env) == 1 and _fused_launches(twin) == 1
    _same_steps(env, twin, (1, 2))
    assert _fused_launches(env) == 2 and _fused_launches(twin) == 2
    env.reset()
    twin.reset()
    assert _fused_launches(env) == 0 and _fused_launches(twin) == 1
    m = np.zeros(B, bool)
    m[MASKED] = True
    env.reset(mask=m)
    assert _fused_launches(env) == 0


# ---- 3. invalidation ---------------------------------------------------------------------------------------------------------------------------
def _whole(e):
    e.set_screens(smooth_screens(B, N, 77))
    return slice(0, B)


def _sub_set(e):
    e.set_screens(smooth_screens(20, N, 78), first=40)
    return slice(40, 60)


def _sub_generate(e):
    sel = np.zeros(B, bool)
    sel[30:50] = True
    e._generate_screens(mask=sel)
    return slice(30, 50)


def _turbulence(e):
    sel = np.zeros(B, bool)
    sel[64:] = True
    e.set_turbulence(0.08, mask=sel)   # (aog_set_turbulence, then those envs' screens drawn at the new value)
    return slice(64, B)


def _tables(e):
    e.tables = dataclasses.replace(e.tables, wfs_coef=e.tables.wfs_coef * 2.0)   # every power x 4
    e._upload_tables()
    return slice(0, B)


@pytest.mark.parametrize("change", [_whole, _sub_set, _sub_generate, _turbulence, _tables],
                         ids=["set_screens_whole", "set_screens_range", "generate_screens_range", "set_turbulence", "tables"])
def test_installing_something_invalidates_the_cache(pair, change):
    torch = _torch()
    env, twin = pair()
    stale = _same_reset(env, twin)
    _same_steps(env, twin, (1,))
    _same_reset(env, twin)              # a hit: the cache is in use
    rows = change(env)
    assert change(twin) == rows
    fresh = _same_reset(env, twin)
    changed = (fresh[1] != stale[1]).any(dim=1).cpu().numpy()
    inside = np.zeros(B, bool)
    inside[rows] = True
    assert changed[inside].all() and not changed[~inside].any()
    _same_steps(env, twin, (2,))
    again = _same_reset(env, twin)      # refilled: hits again with the new observation
    assert torch.equal(again[1], fresh[1])


def test_set_state_invalidates_the_cache(pair):
    torch = _torch()
    env, twin = pair()
    first = _same_reset(env, twin)
    states = [e.get_state() for e in (env, twin)]
    for e in (env, twin):
        e.set_screens(smooth_screens(B, N, 79))
    other = _same_reset(env, twin)      # filled under the other screens
    assert not torch.equal(other[1], first[1])
    for e, st in zip((env, twin), states):
        e.set_state(st)
    back = _same_reset(env, twin)
    assert torch.equal(back[1], first[1]) and torch.equal(back[0], first[0])
    _same_steps(env, twin, (3,))


# ---- 4. masked resets --------------------------------------------------------------------------------------------------------------------------
def test_masked_reset_with_a_valid_cache(pair):
    torch = _torch()
    env, twin = pair()
    flat = _same_reset(env, twin)
    _same_steps(env, twin, (1,))
    before_act = env.get_actuators()
    mask = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
    mask[MASKED] = 1
    m = mask.bool()
    # the library call itself: only the selected rows of the caller's buffers are written
    raw = torch.full((B, 4), -7.0, dtype=torch.float32, device="cuda:0")
    obs = torch.full((B, 4), -7.0, dtype=torch.float16, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert env.lib.aog_reset(env._handle, C.c_void_p(mask.data_ptr()), C.c_void_p(raw.data_ptr()), C.c_void_p(obs.data_ptr()), stream) == 0
    twin.reset(mask=mask)
    assert torch.equal(raw[m], flat[1][m]) and torch.equal(obs[m], flat[0][m])
    assert bool((raw[~m] == -7.0).all()) and bool((obs[~m] == -7.0).all())
    assert torch.equal(raw[m], twin.last_obs_raw[m])
    act = env.get_actuators()
    assert float(act[m].abs().max()) == 0 and torch.equal(act[~m], before_act[~m]) and torch.equal(act, twin.get_actuators())
    # t_render, actuators and screens of every env as the twin's: the saved device state is the same bytes (the host counters too: both
    # calls advanced the observation frame)
    assert torch.equal(_blob(env), _blob(twin))
    _same_steps(env, twin, (2, 3))      # timesteps_per_episode = 3: the unselected envs finish here, the selected ones do not
    # through the Python API: unselected rows are the last observation, which is what the pupil pass writes there
    _same_reset(env, twin, mask=mask)
    _same_steps(env, twin, (4,))


def test_masked_reset_with_an_invalid_cache(pair):
    torch = _torch()
    env, twin = pair()
    for e in (env, twin):
        e.profile(True, every=1, block=1)
    _same_reset(env, twin)
    _same_steps(env, twin, (1,))
    for e in (env, twin):
        e.set_screens(smooth_screens(B, N, 80))
    _fused_launches(env)
    mask = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
    mask[MASKED] = 1
    _same_reset(env, twin, mask=mask)
    assert _fused_launches(env) == 1    # ran the pass and kept nothing: the other envs' mirrors are not flat
    _same_steps(env, twin, (2,))
    _same_reset(env, twin, mask=mask)
    assert _fused_launches(env) == 2
    full = _same_reset(env, twin)       # fills
    assert _fused_launches(env) == 1
    _same_steps(env, twin, (3,))
    _fused_launches(env)
    hit = _same_reset(env, twin)
    assert _fused_launches(env) == 0 and torch.equal(hit[1], full[1])


# ---- 5. handles that must not cache ------------------------------------------------------------------------------------------------------------
def test_semi_dynamic_resets_observe_their_new_screens(pair):
    torch = _torch()
    env, twin = pair(atm_type="semi_dynamic")
    a = _same_reset(env, twin)
    _same_steps(env, twin, (1,))
    b = _same_reset(env, twin)
    assert bool((a[1] != b[1]).any(dim=1).all())


def test_dynamic_handles_never_cache(pair):
    env, twin = pair(atm_type="dynamic", atm_vel=20.0, timesteps_per_episode=2)
    for e in (env, twin):
        e.profile(True, every=1, block=1)
    for ep in range(2):
        _same_reset(env, twin)
        _same_steps(env, twin, (10 * ep + 1, 10 * ep + 2))
    assert _fused_launches(env) == _fused_launches(twin) == 6


def test_detector_resets_draw_fresh_noise(pair):
    torch = _torch()
    env, twin = pair(obs_photons=3e3, obs_read_noise=2.0, obs_background=1.0)
    a = _same_reset(env, twin)
    b = _same_reset(env, twin)
    assert float((a[1] != b[1]).float().mean()) > 0.9
    _same_steps(env, twin, (1,))
    _same_reset(env, twin)
    # detector off: the clean observation may be cached now; on again: noisy frames as the twin's
    for e in (env, twin):
        e.set_detector(None)
    c = _same_reset(env, twin)
    d = _same_reset(env, twin)
    assert torch.equal(c[1], d[1])
    for e in (env, twin):
        e.set_detector(3e3, 2.0, 1.0)
    _same_reset(env, twin)
    _same_reset(env, twin)


def test_reset_with_policy_runs_the_pass(pair):
    torch = _torch()
    from adaptive_optics_gym_amd.rollout import DeviceActor
    from test_gpu_action_noise import _actor

    env, twin = pair()
    for e in (env, twin):
        e.profile(True, every=1, block=1)
    actor = _actor(4, A, 64)
    d1, d2 = DeviceActor(actor, seed=9), DeviceActor(actor, seed=9)
    _same_reset(env, twin)              # the cache is valid from here on
    for ep in range(2):
        (o1, _), p1 = env.reset_with_policy(d1)
        (o2, _), p2 = twin.reset_with_policy(d2)
        assert torch.equal(o1, o2) and torch.equal(p1[0], p2[0]) and torch.equal(p1[2], p2[2])
        r1, _ = env.step_with_policy(d1)
        r2, _ = twin.step_with_policy(d2)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and torch.equal(r1[4]["obs_raw"], r2[4]["obs_raw"])
        # leave the pending action behind: a plain step sequence follows
        for e, d in ((env, d1), (twin, d2)):
            e.step_with_policy(d)
            e.step_with_policy(d)
    assert _fused_launches(env) == _fused_launches(twin) == 1 + 2 * 4


def test_a_mirror_that_does_not_restart_flat_is_not_cached(pair):
    torch = _torch()
    env, twin = pair(flat_mirror_start_per_episode=False)
    a = _same_reset(env, twin)
    _same_steps(env, twin, (1,))
    b = _same_reset(env, twin)          # observes the mirror the step left
    assert bool((a[1] != b[1]).any(dim=1).all())
