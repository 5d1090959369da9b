"""The library's one host packer of the matrix Fourier transform family's split-f16 operand tiles (csrc/mft_host.h, through the host-only
ABI entries ``aog_pack_operand_tiles`` / ``aog_reorder_operand_tiles``) against the independent numpy packers of ``pyramid_host.py``, bit for
bit: both K orders over ragged shapes with and without spare padding, and the re-ordering ``aog_pyramid_gradient`` applies to its tables.
No GPU."""
import itertools

import numpy as np
import pytest

from adaptive_optics_gym_amd import _lib, pyramid_host

ROWS = (1, 31, 32, 33, 50)
KS = (1, 15, 16, 17, 33, 50)
SCALE = 2.0 ** -3            # a non-unit power of two: m * SCALE is exact
K_UNIT = {"natural": 16, "accumulator": 32}   # pack_columns_accumulator lays K out in whole 32s


def _round_up(v, m):
    return -(-v // m) * m


def _matrix(rows, K, seed):
    """complex [rows, K] whose entries x SCALE have magnitudes from 2^-20 to 1, with exact zeros and values exactly halfway between two
    neighbouring halves (ties to even, up and down).  Every component is a float32 value: the packer's split is defined as double -> float
    -> half, but HIP host code is compiled with floating-point contraction on, which lets the compiler merge the two conversions into one
    rounding, and a float64 within float32 rounding of a half tie (one random value in 2^13) then gets the other neighbour as its hi than
    numpy's two steps give.  Both splits carry the value to the same precision; on float32 values the two agree bit for bit, so the
    comparison below holds the layout, the pads and the split itself without depending on what the compiler merges."""
    rng = np.random.default_rng(seed)

    def part():
        v = rng.uniform(0.5, 1.0, (rows, K)).astype(np.float32).astype(np.float64) * 2.0 ** -rng.integers(0, 21, (rows, K)) * rng.choice([-1.0, 1.0], (rows, K))
        flat = v.ravel()
        special = [0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(0.5 + 2.0 ** -12), 2.0 ** -20 * (1 + 2.0 ** -5)]
        where = rng.permutation(flat.size)
        for n, i in enumerate(where[:max(1, flat.size // 3)]):
            flat[i] = special[n % len(special)]
        return flat.reshape(rows, K)

    return (part() + 1j * part()) / SCALE


def _numpy_tiles(m, order, n_blocks, k_pad):
    """m [rows, K] (already scaled) through pyramid_host's packer of that order, as uint16 [n_blocks, k_pad / 16, 4, 64, 8]."""
    if order == "natural":
        t = pyramid_host.pack_rows_natural(m, n_blocks, k_pad)
    else:
        t = pyramid_host.pack_columns_accumulator(m.T, n_blocks, k_pad)
    return np.ascontiguousarray(t).view(np.uint16).reshape(n_blocks, k_pad // 16, 4, 64, 8)


def _position(order, i, k):
    """(block, k-step, lane, slot) of element (i, k): DESIGN.md §5's two orders, written out here a third time on purpose."""
    if order == "natural":
        return i >> 5, k >> 4, (i & 31) + 32 * ((k >> 3) & 1), k & 7
    return i >> 5, k >> 4, (i & 31) + 32 * ((k >> 2) & 1), (k & 3) + 4 * ((k >> 3) & 1)


def test_the_matrices_exercise_the_rounding_cases():
    """What the issue asks of the entries: zeros, hi halves from 2^-20 up to 1, lo halves that are subnormal or zero beside a non-zero hi, and ties."""
    m = _matrix(50, 50, 1) * SCALE
    hi, lo = pyramid_host._split(m.real)
    assert (m.real == 0).any() and (m.imag == 0).any()
    assert np.abs(m.real[m.real != 0]).min() < 2.0 ** -19 and np.abs(m.real).max() > 0.5
    tiny = 2.0 ** -14
    assert ((hi != 0) & (lo == 0)).any() and ((lo != 0) & (np.abs(lo.astype(np.float64)) < tiny)).any()
    assert (m.real == 1.0 + 2.0 ** -11).any() and (hi[m.real == 1.0 + 2.0 ** -11] == 1.0).all()                      # tie -> even (down)
    assert (hi[m.real == 1.0 + 3 * 2.0 ** -11] == np.float16(1.0 + 2.0 ** -9)).all()                                  # tie -> even (up)


@pytest.mark.parametrize("order", ["natural", "accumulator"])
@pytest.mark.parametrize("spare", [False, True], ids=["minimal", "spare"])
def test_pack_matches_the_numpy_packers(order, spare):
    """Every (rows, K): the library's tiles equal pyramid_host's, the pads are zero, and every element of the output is written."""
    for n, (rows, K) in enumerate(itertools.product(ROWS, KS)):
        m = _matrix(rows, K, 100 + n)
        n_blocks, k_pad = _round_up(rows, 32) // 32 + spare, _round_up(K, K_UNIT[order]) + 32 * spare
        out = np.full((n_blocks, k_pad // 16, 4, 64, 8), 0xFFFF, dtype=np.uint16)
        got = _lib.pack_operand_tiles(m, SCALE, order, n_blocks, k_pad, out=out)
        assert got is out and got.dtype == np.uint16
        want = _numpy_tiles(m * SCALE, order, n_blocks, k_pad)
        assert np.array_equal(got, want), (order, rows, K, n_blocks, k_pad)
        used = np.zeros(got.shape, dtype=bool)
        for i, k in itertools.product(range(rows), range(K)):
            b, ks, lane, slot = _position(order, i, k)
            used[b, ks, :, lane, slot] = True
        assert not got[~used].any(), (order, rows, K, "pads must be zero")
        assert used.sum() == 4 * rows * K


# aog_pyramid_gradient's four tables: (source order, destination order) of m1s -> m1s_t, m2s -> m2s_t, b1s -> b1s_t, b2s -> b2s_t
REORDERS = {"m1": ("natural", "accumulator"), "m2": ("accumulator", "natural"), "b1": ("accumulator", "accumulator"), "b2": ("accumulator", "accumulator")}
SIDES = (20, 33, 48, 50)


@pytest.mark.parametrize("table", list(REORDERS))
def test_reorder_gives_the_transposed_matrix_tiles(table):
    """Re-ordering packed tiles equals packing the transposed matrix in the destination order, bit for bit (the split is elementwise), over
    non-square shapes; the destination's shape follows the source's padding the way grad_buffers_fast sizes its tables, so a source K padded
    to an odd number of 16s (rows 33 x K 33 or 48 in natural order) leaves a destination half-block with no source: zeros."""
    src_order, dst_order = REORDERS[table]
    for n, (rows, K) in enumerate(itertools.permutations(SIDES, 2)):
        m = _matrix(rows, K, 500 + n)
        src_blocks, src_k_pad = _round_up(rows, 32) // 32, _round_up(K, K_UNIT[src_order])
        dst_blocks, dst_k_pad = _round_up(src_k_pad, 32) // 32, 32 * src_blocks
        src = _lib.pack_operand_tiles(m, SCALE, src_order, src_blocks, src_k_pad)
        out = np.full((dst_blocks, dst_k_pad // 16, 4, 64, 8), 0xFFFF, dtype=np.uint16)
        got = _lib.reorder_operand_tiles(src, src_order, dst_order, dst_blocks, dst_k_pad, out=out)
        want = _lib.pack_operand_tiles(m.T, SCALE, dst_order, dst_blocks, dst_k_pad)
        assert np.array_equal(got, want), (table, rows, K)
        assert np.array_equal(got, _numpy_tiles(m.T * SCALE, dst_order, dst_blocks, dst_k_pad)), (table, rows, K)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    m = _matrix(4, 4, 9)
    with pytest.raises(_lib.AogError, match="does not fit"):
        _lib.pack_operand_tiles(_matrix(33, 4, 9), SCALE, "natural", 1, 16)
    with pytest.raises(_lib.AogError, match="multiple of 16"):
        _lib.pack_operand_tiles(m, SCALE, "natural", 1, 24)
    out = np.zeros((1, 1, 4, 64, 8), dtype=np.uint16)
    ri = np.ascontiguousarray(np.stack([m.real, m.imag], axis=-1))
    assert lib.aog_pack_operand_tiles(ri.ctypes.data, 4, 4, 1.0, 2, 1, 16, out.ctypes.data) == -1 and b"aog_pack_operand_tiles" in lib.aog_last_error()
    assert lib.aog_pack_operand_tiles(None, 4, 4, 1.0, 0, 1, 16, out.ctypes.data) == -1
    assert lib.aog_reorder_operand_tiles(out.ctypes.data, 0, 1, 16, 1, 1, 8, out.ctypes.data) == -1
