"""The fused pupil pass's launch plan over the shapes the library accepts, on the host: ``aog_fused_plan`` returns what ``aog_create`` and
the launcher compute (``fused_geometry()`` and ``FusedLds`` of csrc/fused_layout.h), and every plan must be launchable — the dynamic LDS fits
a CU in both forms a dynamic handle can take, the proportional chunk split leaves no chunk empty or longer than the LDS was sized for, the
sub-chunk shares add up, and the workgroup map covers every (pixel chunk, env group) once.  No GPU."""
import itertools

import numpy as np
import pytest

from adaptive_optics_gym_amd import _lib, optics_host

LDS_PER_CU = 160 * 1024      # gfx950
BATCHES = (1, 32, 33, 64, 65, 96, 97, 128, 129, 255, 256, 257, 320, 1000, 1024, 4096)
PUPILS = (32, 50, 64, 240, 256, 512)
ACT_DIMS = (3, 16, 17, 32, 33, 64, 65, 100, 128)
OBS_DIMS = (2, 3, 4, 5)


def _n_ap(N):
    return int(optics_host.aperture_mask(N, 0.5).sum())


def _n_tables(o):
    return o * o + 3         # o^2 observation pixels + 3 fiber modes, realified (test_collapsed_tables_reproduce_literal_pipeline)


def wg_map(L, pair, wg_y):
    """k_fused.h's fused_wg_map: workgroup L -> (pixel chunk, env group)."""
    j, xcd = L >> 3, L & 7
    if pair:
        cpr = 64 // wg_y
        r, k, half = j >> 6, j & 31, (j >> 5) & 1
        return (r * cpr + k % cpr) * 8 + xcd, k // cpr + (wg_y >> 1) * half
    return (j // wg_y) * 8 + xcd, j % wg_y


def launched_grid(P, pair, wg_y):
    """fused_inst.hip's launch_tab: the 1-D grid."""
    chunks_per_xcd = (P + 7) // 8
    per_xcd = -(-chunks_per_xcd // (64 // wg_y)) * (64 // wg_y) * wg_y if pair else chunks_per_xcd * wg_y
    return 8 * per_xcd


def assert_map_covers(P, pair, wg_y):
    c, eg = wg_map(np.arange(launched_grid(P, pair, wg_y)), pair, wg_y)
    assert eg.min() >= 0 and eg.max() < wg_y and c.min() >= 0
    real = c < P                                   # (workgroups of chunks past the last one leave at once)
    cells = c[real] * wg_y + eg[real]
    assert cells.size == P * wg_y and np.array_equal(np.sort(cells), np.arange(P * wg_y)), (P, pair, wg_y)


def check_split(n_ptiles, P, tpc, heavy, wp):
    """The chunks [c n / P, (c + 1) n / P) and each one's sub-chunks (k_fused_tab)."""
    edges = np.arange(P + 1, dtype=np.int64) * n_ptiles // P
    nt = np.diff(edges)
    assert edges[0] == 0 and edges[-1] == n_ptiles
    assert nt.min() >= 1, "an empty chunk"
    assert nt.max() <= tpc, "a chunk longer than the science rows the LDS holds"
    if heavy > 0:                                  # asymmetric pairs: sub-chunk 0 takes min(nt, (nt heavy + 512) >> 10), sub-chunk 1 the rest
        assert wp == 2
        n_heavy = np.minimum(nt, (nt * heavy + 512) >> 10)
        light = nt - n_heavy
        assert n_heavy.min() >= 1 and light.min() >= 0 and np.array_equal(n_heavy + light, nt)
    else:                                          # interleaved: sub-chunk w takes tiles t0 + w, t0 + w + wp, ...
        shares = [np.where(nt > w, (nt - w + wp - 1) // wp, 0) for w in range(wp)]
        assert np.array_equal(sum(shares), nt)


def check_plan(p, B, n_ap, A, tables, dynamic, pixel_chunks, four_wave):
    """Returns a reason the plan could not launch, or None.  Raises for anything else that is wrong with it."""
    n_ptiles, n_etiles = -(-n_ap // 32), 2 * (-(-B // 64))
    assert (p["n_ptiles"], p["n_etiles"]) == (n_ptiles, n_etiles)
    assert p["A_pad"] >= A and p["MRW"] >= tables and p["A_pad"] in (16, 32, 64, 128) and p["MRW"] in (7, 12, 20, 28)
    assert p["waves"] in (4, 8) and p["we"] in (1, 2, 4) and p["waves"] % p["we"] == 0
    if four_wave or n_etiles < 4:
        assert p["waves"] == 4
    assert (p["heavy"] > 0) == (p["waves"] == 8)
    assert p["we"] * p["wg_y"] >= n_etiles > p["we"] * (p["wg_y"] - 1)
    assert 1 <= p["chunks_x"] <= n_ptiles
    assert p["tpc"] == -(-n_ptiles // p["chunks_x"])
    assert p["n_chunks"] == p["chunks_x"] * p["waves"] // p["we"]
    if p["pair"]:
        assert p["wg_y"] % 2 == 0 and 64 % p["wg_y"] == 0 and p["waves"] == 4
    if pixel_chunks > 0:
        assert p["chunks_x"] >= min(pixel_chunks, n_ptiles)    # (more only where the caller's chunks would not fit the LDS)
    if not dynamic:
        assert p["lds_ring"] == p["lds_tiles"]
    assert p["lds_ring"] >= p["lds_tiles"] > 0
    if max(p["lds_tiles"], p["lds_ring"]) > LDS_PER_CU:
        return "%d waves need %d / %d bytes of LDS" % (p["waves"], p["lds_tiles"], p["lds_ring"])
    return None


def test_every_accepted_shape_has_a_launchable_plan():
    n_aps = {N: _n_ap(N) for N in PUPILS}
    assert n_aps[32] == 812 and n_aps[64] == 3228          # 26 pixel tiles, the last with 12 pixels; 101 tiles
    unlaunchable, splits, maps = {}, set(), set()
    for dynamic, o, A, N, B in itertools.product((False, True), OBS_DIMS, ACT_DIMS, PUPILS, BATCHES):
        n_ap, tables = n_aps[N], _n_tables(o)
        n_ptiles = -(-n_ap // 32)
        for pixel_chunks, four_wave in itertools.product((0, 1, 3, n_ptiles, n_ptiles + 5), (False, True)):
            p = _lib.fused_plan(B, n_ap, A, tables, dynamic, pixel_chunks, four_wave)
            why = check_plan(p, B, n_ap, A, tables, dynamic, pixel_chunks, four_wave)
            if why:
                row = ("dynamic" if dynamic else "static", p["A_pad"], p["MRW"], p["waves"])
                unlaunchable.setdefault(row, []).append((B, N, A, o, pixel_chunks, four_wave, why))
                continue
            splits.add((n_ptiles, p["chunks_x"], p["tpc"], p["heavy"], p["waves"] // p["we"]))
            maps.add((p["chunks_x"], p["pair"], p["wg_y"]))
    for s in splits:
        check_split(*s)
    for m in maps:
        assert_map_covers(*m)
    assert {m[1] for m in maps} == {0, 1} and {1, 2, 3, 8, 32} <= {m[2] for m in maps}    # (wg_y = 4 needs B = 512: the map test below)
    report = "\n".join("%s A_pad=%d tables=%d waves=%d: %d shapes, e.g. B=%d N=%d act_dim=%d o=%d pixel_chunks=%d four_wave=%s: %s"
                       % (row + (len(v),) + v[0]) for row, v in sorted(unlaunchable.items()))
    assert not unlaunchable, "plans that cannot launch (atmosphere, A_pad, tables, waves):\n" + report


@pytest.mark.parametrize("pair,wg_y", [(0, w) for w in (1, 2, 3, 4, 8, 32)] + [(1, w) for w in (2, 4, 8, 32, 64)])   # (paired: even divisors of 64)
def test_workgroup_map_covers_every_chunk_and_env_group_once(pair, wg_y):
    for P in (1, 2, 7, 8, 9, 26, 64, 101, 256, 513):
        assert_map_covers(P, pair, wg_y)


def test_pinned_baseline_geometries():
    """The two shapes csrc/fused_layout.h pins with static_assert (BASELINE configs 2 and 3: N = 256 has 51468 aperture pixels), seen through
    the call: a change of any number changes the order of the float64 sums."""
    assert _n_ap(256) == 51468
    want = dict(we=4, waves=8, heavy=672, wg_y=8, pair=0, chunks_x=32, tpc=51, n_chunks=64, valu_qpc=72, valu_chunks=179, lds_tiles=6528, lds_ring=6528)
    p = _lib.fused_plan(1024, 51468, 64, 7)
    assert {k: p[k] for k in want} == want
    want = dict(we=4, waves=8, heavy=672, wg_y=32, pair=0, chunks_x=8, tpc=202, n_chunks=16, valu_qpc=272, valu_chunks=48, lds_tiles=156928,
                lds_ring=156928)
    p = _lib.fused_plan(4096, 51468, 64, 28)
    assert {k: p[k] for k in want} == want


def test_forms_of_the_shapes_that_outgrow_eight_waves():
    """Variants whose 8-wave fixed areas leave no room for a chunk keep 4-wave workgroups at every batch size; the 128-mode static handle
    at o = 2, whose real layout fits, keeps 8 waves."""
    n_ap = _n_ap(32)
    for dynamic, A, o in ((False, 100, 3), (False, 100, 4), (False, 100, 5), (True, 64, 3), (True, 16, 5), (True, 20, 4), (True, 20, 5),
                          (True, 64, 4), (True, 64, 5), (True, 100, 2), (True, 100, 3), (True, 100, 4), (True, 100, 5)):
        for B in (65, 128, 1024):
            p = _lib.fused_plan(B, n_ap, A, _n_tables(o), dynamic)
            assert (p["waves"], p["we"], p["heavy"]) == (4, 4, 0), (dynamic, A, o, B)
    for dynamic, A, o in ((False, 100, 2), (False, 64, 5), (True, 64, 2), (True, 16, 4), (True, 20, 3)):
        assert _lib.fused_plan(128, n_ap, A, _n_tables(o), dynamic)["waves"] == 8, (dynamic, A, o)
    p = _lib.fused_plan(128, n_ap, 100, 7)
    assert (p["chunks_x"], p["tpc"], p["n_chunks"], p["lds_tiles"]) == (26, 1, 52, 131200)


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    out = (np.zeros(16, dtype=np.int32)).ctypes
    assert lib.aog_fused_plan(0, 812, 16, 7, 0, 0, 0, out) == -1 and b"aog_fused_plan" in lib.aog_last_error()
    assert lib.aog_fused_plan(4, 812, 16, 7, 0, 0, 0, None) == -1
    assert lib.aog_fused_plan(4, 812, 129, 7, 0, 0, 0, out) == -4 and b"act_dim <= 128" in lib.aog_last_error()
    assert lib.aog_fused_plan(4, 812, 16, 29, 0, 0, 0, out) == -4
