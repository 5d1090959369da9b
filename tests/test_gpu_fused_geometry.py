"""k_fused_tab over its launch forms (run with -m gpu on an MI355X): 4- and 8-wave workgroups, 1 to 4 workgroups per pixel chunk, both
workgroup maps, clamped env tiles, one-tile and uneven chunks, every LDS layout (operands above 64 modes or ring-direct, transpose tiles, a
float64 plane per wave at o >= 3) — each against the float64 numpy oracle on sampled envs, with test_gpu_parity.py's comparison and its
tolerances (1e-5 relative before the float16 cast, 1 ulp after, nulls below 1e-3 of the peak held absolutely).

N = 32 has 812 aperture pixels: 26 pixel tiles, the last with 12 pixels, and at B >= 65 one tile per chunk (the light sub-chunk of an 8-wave
workgroup is empty).  N = 64 has 3228: 101 tiles."""
import numpy as np
import pytest

from helpers import actions_for, run_oracle, smooth_screens
from test_gpu_parity import _assert_obs_close, _compare, _drive, _ring_direct_oracle_replay, _torch

pytestmark = pytest.mark.gpu

T_STEPS = 2
SCREEN_SEED, ACTION_SEED = 61, 40
_SCREENS, _ORACLE = {}, {}


def _screens(N, B):
    """smooth_screens draws env after env from one stream, so env b has the same screen in every batch of a pupil size."""
    have = _SCREENS.get(N)
    if have is None or have.shape[0] < B:
        have = _SCREENS[N] = smooth_screens(max(B, 160), N, SCREEN_SEED + N)
    return have[:B]


def _actions(B, A):
    return np.stack([actions_for(B, A, ACTION_SEED + s) for s in range(T_STEPS)])      # (row b does not depend on B either)


def _sampled(B):
    """First, the two sides of the first env-tile boundary, last, and the first env of the last real env tile (the last workgroup's): a wrong
    env tile, a wrong clamp of the padded tiles or a wrong env group shows in one of them."""
    return sorted({0, 31, 32, B - 1, (B - 1) // 32 * 32} & set(range(B)))


def _oracle(N, ids, scr, acts, kw):
    """The oracle's reset and steps of the sampled envs, one env at a time and computed once per (shape, env)."""
    per_env = []
    for b in ids:
        key = (N, b) + tuple(sorted(kw.items()))
        if key not in _ORACLE:
            _ORACLE[key] = run_oracle(scr[b:b + 1], acts[:, b:b + 1], **kw)
        per_env.append(_ORACLE[key])
    return {k: np.concatenate([p[k] for p in per_env], axis=0 if k == "obs0" else 1) for k in per_env[0]}


def _plan(B, N, A, o, dynamic=False, pixel_chunks=0, four_wave=False):
    from adaptive_optics_gym_amd import _lib, optics_host

    return _lib.fused_plan(B, int(optics_host.aperture_mask(N, 0.5).sum()), A, o * o + 3, dynamic, pixel_chunks, four_wave)


def _kw(A, o, rew="strehl_ratio"):
    return dict(act_type="num_actuators" if A > 21 else "zernike", act_dim=A, obs_dim=o, rew_type=rew, timesteps_per_episode=T_STEPS)


def _run_case(B, N, A, o, rew="strehl_ratio", pixel_chunks=0, want=None, four_wave=False):
    """reset + two steps (the second ends the episode) of the matrix-core kernel against the oracle on the sampled envs; `want`: fields of
    the launch plan that the case is there for, checked against the plan call and, through the slab count, against the handle."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    plan = _plan(B, N, A, o, False, pixel_chunks, four_wave)
    for k, v in (want or {}).items():
        assert plan[k] == v, (k, plan)
    kw = _kw(A, o, rew)
    scr, acts, ids = _screens(N, B), _actions(B, A), _sampled(B)
    ref = _oracle(N, ids, scr, acts, kw)
    env = BatchedAOEnv(B, "cuda:0", num_pupil_pixels=N, screens=scr, kernel="mfma", pixel_chunks=pixel_chunks, verbose=False, **kw)
    assert env.info.kernel == 2 and env.info.pixel_chunks == plan["n_chunks"] and env.info.num_envs_padded == 32 * plan["n_etiles"]
    got = _drive(env, acts, torch)
    assert env.device_status() == 0
    env.close()
    got = {k: (v[:, ids] if k != "obs0" else v[ids]) for k, v in got.items()}
    _compare(got, ref, rew == "strehl_ratio")


@pytest.mark.parametrize("B,wg_y", [(65, 1), (129, 2), (257, 3)])
def test_env_side_forms(B, wg_y):
    """8-wave workgroups of four env tiles, 1 to 3 of them per pixel chunk; B = 257 pads to 320 envs: its last workgroup has two real env
    tiles (the second with one env) and two clamped ones."""
    _run_case(B, 32, 16, 2, want=dict(waves=8, we=4, wg_y=wg_y, pair=0, heavy=672, chunks_x=26, tpc=1))


@pytest.mark.parametrize("o", [2, 3, 4, 5])
@pytest.mark.parametrize("A", [6, 20, 64, 100])
def test_operand_and_table_variants_above_64_envs(A, o):
    """B = 70 (four env tiles, the third with 6 envs, the fourth clamped): every table count with operands in registers (A <= 64) and in LDS
    (A = 100).  Static handles: A = 100 at o >= 3 runs 4-wave workgroups because eight waves' operands and float64 planes exceed the LDS."""
    waves = 4 if (A > 64 and o >= 3) else 8
    rew = "smf_ssim" if (o >= 3 and (A in (6, 64)) == (o % 2 == 1)) else "strehl_ratio"     # half of the o >= 3 cases
    _run_case(70, 32, A, o, rew=rew, want=dict(waves=waves, we=4, wg_y=1, chunks_x=26, n_chunks=26 * waves // 4))


@pytest.mark.parametrize("o,pixel_chunks,tpc", [(2, 1, 101), (2, 3, 34), (2, 5, 21), (2, 101, 1), (5, 1, 101), (5, 3, 34)])
def test_chunk_edges(o, pixel_chunks, tpc):
    """The caller's chunk counts at 101 tiles: all tiles in one chunk, uneven chunks (33 / 34 / 34 tiles, heavy share 22 of each), one tile
    per chunk; o = 5 folds its float64 plane every 13 tiles of a long chunk."""
    if pixel_chunks == 3:
        nt = np.diff(np.arange(4) * 101 // 3)
        assert nt.tolist() == [33, 34, 34] and (np.minimum(nt, (nt * 672 + 512) >> 10)).tolist() == [22, 22, 22]
    _run_case(129, 64, 64, o, rew="smf_ssim" if o == 5 else "strehl_ratio", pixel_chunks=pixel_chunks,
              want=dict(waves=8, wg_y=2, chunks_x=pixel_chunks, tpc=tpc))


@pytest.mark.parametrize("o", [2, 5])
@pytest.mark.parametrize("B,wg_y,pair", [(256, 2, 1), (512, 4, 1), (320, 3, 0)])
def test_forced_four_wave_form(monkeypatch, B, wg_y, pair, o):
    """AOG_FUSED_4WAVE above 64 envs: 4-wave workgroups of four env tiles, several per pixel chunk, through the paired workgroup map where
    wg_y is an even divisor of 64 and through the plain one elsewhere."""
    monkeypatch.setenv("AOG_FUSED_4WAVE", "1")
    _run_case(B, 32, 16, o, rew="smf_ssim" if o == 5 else "strehl_ratio", four_wave=True,
              want=dict(waves=4, we=4, heavy=0, wg_y=wg_y, pair=pair, chunks_x=26, n_chunks=26))


@pytest.mark.parametrize("A,o", [(16, 5), (64, 3), (100, 2), (100, 5)])
def test_ring_direct_four_wave_forms(A, o):
    """Dynamic atmosphere read ring-direct at B = 70: the variants whose eight waves' operands, transpose tiles and float64 planes exceed the
    LDS, in the 4-wave form they run in, against the oracle's layer fed the same normals; two episodes of two steps."""
    B, N = 70, 64
    plan = _plan(B, N, A, o, dynamic=True)
    assert (plan["waves"], plan["we"], plan["wg_y"], plan["chunks_x"], plan["tpc"]) == (4, 4, 1, 101, 1) and plan["lds_ring"] <= 160 * 1024
    n_chunks = _ring_direct_oracle_replay(N, 70.0, B=B, A=A, o=o, T=2, steps=4, ids=_sampled(B))   # (asserts info.reserved and device_status)
    assert n_chunks == plan["n_chunks"]


@pytest.mark.parametrize("B,A,o,four_wave,form", [(70, 64, 5, False, (8, 1, 0)), (70, 100, 3, False, (4, 1, 0)), (257, 16, 2, False, (8, 3, 0)),
                                                  (256, 16, 2, True, (4, 2, 1))])
def test_every_env_agrees_with_the_float64_kernel(monkeypatch, B, A, o, four_wave, form):
    """One shape per form: the matrix-core kernel's observations of ALL envs, not only the sampled ones, against the float64 device kernel."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    if four_wave:
        monkeypatch.setenv("AOG_FUSED_4WAVE", "1")
    plan = _plan(B, 32, A, o, four_wave=four_wave)
    assert (plan["waves"], plan["wg_y"], plan["pair"]) == form
    kw = dict(num_pupil_pixels=32, screens=_screens(32, B), verbose=False, **_kw(A, o))
    acts = torch.from_numpy(_actions(B, A)).cuda()
    ref = BatchedAOEnv(B, "cuda:0", precision="fp64", **kw)
    env = BatchedAOEnv(B, "cuda:0", kernel="mfma", **kw)
    assert env.info.kernel == 2 and env.info.pixel_chunks == plan["n_chunks"]
    ref.reset(); env.reset()
    _assert_obs_close(env.last_obs_raw.cpu().numpy(), ref.last_obs_raw.cpu().numpy())
    for t in range(T_STEPS):
        r_info, info = ref.step(acts[t])[4], env.step(acts[t])[4]
        _assert_obs_close(info["obs_raw"].cpu().numpy(), r_info["obs_raw"].cpu().numpy())
        np.testing.assert_allclose(info["power"].cpu().numpy(), r_info["power"].cpu().numpy(), rtol=1e-5)
    assert env.device_status() == 0
    ref.close(); env.close()
