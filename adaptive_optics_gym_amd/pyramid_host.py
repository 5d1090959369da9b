"""Host tables of the modulated pyramid wavefront sensor (``aog_upload_pyramid``; the model is DESIGN.md §5, "Pyramid sensor").

float64 numpy: the focal sample grid, the forward matrices m1_j / m2_j of every modulation point (the tilt folded in), the back matrices
b1 / b2 of both halves of the window, the valid-pixel mask, and the split-f16 operand tiles the matrix-core passes read.  Lengths are in
pupil pixels (centred: pixel y sits at y - (N - 1) / 2), focal positions in lambda_wfs / D."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SAMPLES_RANGE = (8, 64)     # w_q
PIXELS_RANGE = (8, 64)      # n_s
MAX_MOD = 32
MOD_MARGIN = 1.0            # lambda / D between the modulation circle and the edge of the window


def check_arguments(n_pupil, samples, q, pixels, n_mod, r_mod):
    """``ValueError`` for anything the sensor is not built for; returns the arguments as (w_q, q, n_s, n_mod, r_mod)."""
    def whole(v, name):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"pyramid: {name} must be a whole number, got {v!r}")
        return int(v)

    wq, q, ns, n_mod = whole(samples, "samples"), whole(q, "q"), whole(pixels, "pixels"), whole(n_mod, "n_mod")
    r_mod = float(r_mod)
    if not SAMPLES_RANGE[0] <= wq <= SAMPLES_RANGE[1]:
        raise ValueError(f"pyramid: samples = {wq} outside {SAMPLES_RANGE[0]} .. {SAMPLES_RANGE[1]} (focal samples per quadrant side)")
    if q < 1:
        raise ValueError(f"pyramid: q = {q} must be at least 1 sample per lambda/D")
    if not PIXELS_RANGE[0] <= ns <= min(PIXELS_RANGE[1], int(n_pupil)):
        raise ValueError(f"pyramid: pixels = {ns} outside {PIXELS_RANGE[0]} .. min({PIXELS_RANGE[1]}, num_pupil_pixels = {n_pupil})")
    if not 1 <= n_mod <= MAX_MOD:
        raise ValueError(f"pyramid: n_mod = {n_mod} outside 1 .. {MAX_MOD}")
    if not np.isfinite(r_mod) or r_mod < 0:
        raise ValueError(f"pyramid: r_mod = {r_mod} must be finite and >= 0")
    if not r_mod + MOD_MARGIN < wq / q:
        raise ValueError(f"pyramid: r_mod + {MOD_MARGIN} = {r_mod + MOD_MARGIN} must stay below the half field of view samples / q = {wq / q} lambda/D")
    return wq, q, ns, n_mod, r_mod


def sample_grid(samples, q):
    """k_i = (i + 1/2 - w/2) / q, i = 0 .. w - 1, w = 2 samples: centred on the pyramid tip, no sample on an edge."""
    w = 2 * int(samples)
    return (np.arange(w) + 0.5 - w / 2) / float(q)


def modulation_points(n_mod, r_mod):
    """kappa [n_mod, 2] = r_mod (cos, sin)(2 pi (j + 1/2) / n_mod): (x, y) in lambda/D."""
    a = 2 * np.pi * (np.arange(int(n_mod)) + 0.5) / int(n_mod)
    return float(r_mod) * np.stack([np.cos(a), np.sin(a)], axis=1)


def detector_axis(n_pupil, pixels):
    """Centres of the detector pixels in centred pupil pixels: pitch N / n_s, symmetric about the pupil's centre."""
    return (np.arange(int(pixels)) + 0.5 - pixels / 2) * (n_pupil / pixels)


def valid_pixels(n_pupil, pixels):
    """[n_s, n_s] bool: the detector pixels whose centre lies inside the aperture."""
    c = detector_axis(n_pupil, pixels)
    return c[:, None] ** 2 + c[None, :] ** 2 <= (n_pupil / 2) ** 2


@dataclass
class PyramidTables:
    n_pupil: int
    n_ap: int
    samples: int            # w_q
    q: int
    pixels: int             # n_s
    n_mod: int
    r_mod: float
    k: np.ndarray           # [w]
    kappa: np.ndarray       # [n_mod, 2] (x, y)
    m1: np.ndarray          # [n_mod, w, N] complex: rows k_y, columns y
    m2: np.ndarray          # [n_mod, N, w] complex: rows x, columns k_x
    b1: np.ndarray          # [2, n_s, w] complex: half 0 = k < 0, zero outside the half
    b2: np.ndarray          # [2, w, n_s] complex
    valid_mask: np.ndarray  # [n_s, n_s] bool
    valid: np.ndarray       # [n_valid] int32 = y n_s + x of the valid pixels, ascending

    @property
    def window(self):
        return 2 * self.samples

    @property
    def n_valid(self):
        return int(self.valid.size)


def pyramid_tables(n_pupil, n_ap, samples, q=2, pixels=32, n_mod=8, r_mod=3.0) -> PyramidTables:
    N = int(n_pupil)
    wq, q, ns, n_mod, r_mod = check_arguments(N, samples, q, pixels, n_mod, r_mod)
    w = 2 * wq
    k = sample_grid(wq, q)
    kappa = modulation_points(n_mod, r_mod)
    y = np.arange(N) - (N - 1) / 2
    amp = 1.0 / np.sqrt(float(n_ap))
    m1 = np.stack([np.exp(-2j * np.pi * np.outer(k - kap[1], y) / N) * amp for kap in kappa])
    m2 = np.stack([np.exp(-2j * np.pi * np.outer(y, k - kap[0]) / N) * amp for kap in kappa])
    yd = detector_axis(N, ns)
    back = np.exp(2j * np.pi * np.outer(yd, k) / N) * np.sqrt(1.0 / q)     # [n_s, w]
    b1 = np.zeros((2, ns, w), dtype=np.complex128)
    b1[0, :, :wq] = back[:, :wq]
    b1[1, :, wq:] = back[:, wq:]
    b2 = np.ascontiguousarray(b1.transpose(0, 2, 1))
    mask = valid_pixels(N, ns)
    return PyramidTables(n_pupil=N, n_ap=int(n_ap), samples=wq, q=q, pixels=ns, n_mod=n_mod, r_mod=r_mod, k=k, kappa=kappa, m1=m1, m2=m2, b1=b1,
                         b2=b2, valid_mask=mask, valid=np.flatnonzero(mask.ravel()).astype(np.int32))


# ------------------------------------------------------------------------------------------------
# split-f16 operand tiles (csrc/k_focal.h: one tile = [re hi, re lo, im hi, im lo][lane 64][8 f16])
# ------------------------------------------------------------------------------------------------
def power_of_two_scale(amplitude):
    """The power of two that brings components of magnitude <= amplitude into [.., 1): 2^-(floor(log2 amplitude) + 1)."""
    return float(2.0 ** -(np.floor(np.log2(amplitude)) + 1))


def _split(x):
    """hi = x rounded to f16, lo = x - hi rounded to f16 (through float32, as the library's own packer rounds)."""
    hi = x.astype(np.float32).astype(np.float16)
    lo = (x - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    return hi, lo


def _tiles(values):
    """complex [..., 64, 8] -> float16 [..., 4, 64, 8]"""
    rh, rl = _split(values.real)
    ih, il = _split(values.imag)
    return np.stack([rh, rl, ih, il], axis=-3)


def pack_rows_natural(m, n_blocks, k_pad):
    """The m1s layout: m [n, K] -> [n_blocks][k_pad / 16] tiles; lane l = row 32 b + (l & 31), slot j = column 16 ks + 8 (l >> 5) + j."""
    n, K = m.shape
    full = np.zeros((n_blocks * 32, k_pad), dtype=np.complex128)
    full[:n, :K] = m
    lane, slot = np.arange(64), np.arange(8)
    b, ks = np.arange(n_blocks), np.arange(k_pad // 16)
    row = 32 * b[:, None, None, None] + (lane & 31)[None, None, :, None]
    col = 16 * ks[None, :, None, None] + 8 * (lane >> 5)[None, None, :, None] + slot[None, None, None, :]
    return np.ascontiguousarray(_tiles(full[row, col]))


def pack_columns_accumulator(m, n_blocks, k_pad):
    """The m2s layout: m [K, n] -> [n_blocks][k_pad / 32][2] tiles; lane l = column 32 b + (l & 31), slot j of k-step (t, s) = row
    32 t + (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 8 s + j — the order a matrix-core accumulator holds its rows."""
    K, n = m.shape
    full = np.zeros((k_pad, n_blocks * 32), dtype=np.complex128)
    full[:K, :n] = m
    lane, slot = np.arange(64), np.arange(8)
    b, t, s = np.arange(n_blocks), np.arange(k_pad // 32), np.arange(2)
    r = 8 * s[:, None] + slot[None, :]                                               # [2, 8]
    inner = (r & 3) + 8 * (r >> 2)                                                   # [2, 8]
    row = 32 * t[None, :, None, None, None] + inner[None, None, :, None, :] + 4 * (lane >> 5)[None, None, None, :, None]
    col = 32 * b[:, None, None, None, None] + (lane & 31)[None, None, None, :, None]
    row, col = np.broadcast_arrays(row, col)
    return np.ascontiguousarray(_tiles(full[row, col]))


def packed_operands(t: PyramidTables):
    """The tables as the fast kernels read them: dict of uint16 arrays (IEEE half bits) m1s, m2s, b1s, b2s and the float factors
    fwd_unscale, back_unscale that undo the powers of two the pairs were scaled by."""
    N, w, ns = t.n_pupil, t.window, t.pixels
    nvb, nsb = -(-w // 32), -(-ns // 32)
    nxp, nyp = -(-N // 128) * 128, -(-N // 16) * 16
    sf = power_of_two_scale(1.0 / np.sqrt(float(t.n_ap)))
    sb = power_of_two_scale(np.sqrt(1.0 / t.q))
    m1s = np.stack([pack_rows_natural(t.m1[j] * sf, nvb, nyp) for j in range(t.n_mod)])
    m2s = np.stack([pack_columns_accumulator(t.m2[j] * sf, nvb, nxp) for j in range(t.n_mod)])
    b1s = np.stack([pack_columns_accumulator(t.b1[h].T * sb, nsb, nvb * 32) for h in range(2)])
    b2s = np.stack([pack_columns_accumulator(t.b2[h] * sb, nsb, nvb * 32) for h in range(2)])
    as_bits = lambda a: np.ascontiguousarray(a).view(np.uint16)
    return dict(m1s=as_bits(m1s), m2s=as_bits(m2s), b1s=as_bits(b1s), b2s=as_bits(b2s), fwd_unscale=1.0 / (sf * sf), back_unscale=1.0 / (sb * sb))
