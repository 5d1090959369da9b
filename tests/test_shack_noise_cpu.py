"""The host restatement of the Shack-Hartmann camera's photon-noise stream (tests/shack_noise_reference.py), without a GPU: its counters
against a plain scalar recomputation, the use of every Philox word at most once, lines beyond 2^32, and what a replay can see — each wrong
key of ``wrong_keys`` moves more than half of the counts, and the share of values a host cannot decide stays under the cap the GPU test
allows."""
import numpy as np
import pytest

import shack_noise_reference as sn
from actor_reference import philox4x32_10

SEED = 0x1234567890ABCDEF
SIZES = [128, 240, 512]


def _rl(N):
    """Lines of 2N = LW RL of the pruned passes: the separable route's sep_rl."""
    return 2 * N // sn.lane_width(N)


def _scalar_word(N, ge, y, x, seed, call, sep_rl, second):
    """One pixel's word from Python integers, k_shack.h's sh_noisy_value read line by line."""
    lw = 60 if (N % 64 != 0 and N % 60 == 0) else 64
    if sep_rl:
        line, r = (ge * N + x) * 64 + (y % sep_rl), y // sep_rl
    else:
        line, r = (ge * N + y) * 64 + (x % lw), x // lw
    assert line < 1 << 64
    c = [line & 0xFFFFFFFF, (line >> 32) ^ ((r >> 2) << 20) ^ (0x80000000 if second else 0), call, 0x50155]
    assert all(0 <= v < 1 << 32 for v in c)
    w = philox4x32_10([np.uint64(v) for v in c], [np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)])
    return int(w[r & 3]), c


def _probe_pixels(N, sep_rl):
    """Corners, the last pixel of lane-index 0 and the first of 1, the first pixel of group 1 (where the size has one), the last pixel —
    along the axis the form's lane index runs on, at the first, a middle and the last position of the other axis."""
    step = sep_rl if sep_rl else sn.lane_width(N)
    along = sorted({0, step - 1, step, min(4 * step, N - 1), N - 1})
    other = [0, N // 2 + 1, N - 1]
    return [((a, o) if sep_rl else (o, a)) for a in along for o in other]   # (y, x)


@pytest.mark.parametrize("form", ["row", "separable"])
@pytest.mark.parametrize("N", SIZES)
def test_counters_match_a_scalar_recomputation_and_no_word_is_used_twice(N, form):
    sep_rl = _rl(N) if form == "separable" else 0
    env_ids = [0, 5]
    call = 7
    for second in (False, True):
        w = sn.sh_words(N, env_ids, SEED, call, sep_rl, second)
        assert w.shape == (2, N, N) and w.dtype == np.uint32
        for e, ge in enumerate(env_ids):
            for y, x in _probe_pixels(N, sep_rl):
                want, _ = _scalar_word(N, ge, y, x, SEED, call, sep_rl, second)
                assert int(w[e, y, x]) == want, (N, form, second, ge, y, x)
    line, r = sn.pixel_lines(N, env_ids, sep_rl)
    line, r = np.broadcast_arrays(line, r)
    assert int(line.max()) < 1 << 40
    calls = line.astype(np.uint64) * np.uint64(8) + (r >> 2).astype(np.uint64)   # one Philox call (of each of the two `second` values)
    _, per_call = np.unique(calls.ravel(), return_counts=True)
    assert per_call.max() <= 4
    words = calls * np.uint64(4) + (r & 3).astype(np.uint64)
    assert np.unique(words.ravel()).size == words.size, "two pixels take the same word of the same call"
    n_groups = int((r >> 2).max()) + 1
    assert n_groups == ((N // (sep_rl or sn.lane_width(N)) + 3) // 4)
    # the groups' and the flag's bits stay clear of the line's high word for every env a handle can hold (2^20 envs of 512 rows: 2^35)
    assert (n_groups - 1) << 20 < 0x80000000


def test_line_beyond_32_bits_reaches_the_high_counter_word():
    N, ge, call = 512, 1 << 20, 2
    for sep_rl in (0, _rl(N)):
        far = sn.sh_words(N, [ge], SEED, call, sep_rl)
        near = sn.sh_words(N, [0], SEED, call, sep_rl)
        for y, x in _probe_pixels(N, sep_rl):
            want, c_far = _scalar_word(N, ge, y, x, SEED, call, sep_rl, False)
            _, c_near = _scalar_word(N, 0, y, x, SEED, call, sep_rl, False)
            assert int(far[0, y, x]) == want
            assert c_far[0] == c_near[0] and c_far[1] == c_near[1] ^ (1 << 3)   # line = ge N 64 + ... = 2^35 + the line of env 0
        assert np.mean(far != near) > 0.999


def _field(E, N):
    lam = sn.lam_field(E, N)
    assert lam.min() == 0.0 and 1e-3 <= lam[lam > 0].min() < 2e-3 and 5e3 < lam.max() <= 1e4
    return lam


@pytest.mark.parametrize("N,form", [(300, "row"), (512, "row"), (128, "separable"), (240, "separable")])
def test_every_wrong_key_moves_most_counts(N, form):
    """What the GPU replay leans on: a device drawing under any of these keys could not pass an exact comparison with the right one."""
    sep_rl = _rl(N) if form == "separable" else 0
    base, call = 16, 3
    ids = base + np.arange(1)
    lam = _field(1, N)
    right, _ = sn.noisy_image(lam, ids, SEED, call, sep_rl)
    _, r = sn.pixel_lines(N, ids, sep_rl)
    assert int((r >> 2).max()) >= 1, "the size must reach group 1"
    keys = sn.wrong_keys(N, sep_rl, base)
    assert len(keys) == (5 if sep_rl else 6)
    for name, key in keys.items():
        wrong, _ = sn.noisy_image(lam, ids, SEED, call, sep_rl, key)
        where = lam >= 1.0
        if name == "group_forced_to_0":
            where = where & np.broadcast_to((r >> 2) >= 1, lam.shape)
        moved = float(np.mean(wrong[where] != right[where]))
        print(f"N {N} {form}: {name} moves {moved:.3f} of {int(where.sum())} counts")
        assert moved > 0.5, name
        if name == "second_flag_dropped":
            assert np.array_equal(wrong[lam < 12.0], right[lam < 12.0])   # (faint pixels never draw the second call)


def test_undecidable_share_stays_under_the_cap():
    """The host alone, on the GPU test's field at n = 320 (seed 77, call 3), under the LW = 64 key the size takes and under the LW = 60 one."""
    lam = _field(2, 320)
    for key in (sn.KEY, sn.KEY._replace(lw=60)):
        n, und = sn.noisy_image(lam, [0, 1], 77, 3, 0, key)
        share = float(und.mean())
        print(f"lane width {key.lw or 64}: {int(und.sum())} of {und.size} flagged ({share:.2e})")
        assert share <= 1e-3
        assert np.all(n >= 0) and np.all(n == np.rint(n)) and np.all(n[lam == 0.0] == 0)
