"""Host restatement of ``aog_install_layer_sum_cone`` (include/aogym_cone.h) in numpy float64, written from the header's text: per axis
``s0 = floor(s); r = s - s0; k = m - 1; e = k (i - ctr); q = e + r; q0 = floor(q); f = q - q0; g = 1 - f``, first index ``i + s0 + q0``, the
bilinear read in the sightline header's brackets,
then the source sum, the modal terms, the mean in its fixed order and the front's two stores exactly as tests/sightline_reference.py
states them (imported, not restated).  numpy's float64 ``*``, ``+``, ``-`` and ``floor`` are single correctly rounded operations and
nothing here is fused, so a float64 front must match ``psi64`` bit for bit."""
import numpy as np

import disturbance_reference as dref
import layered_reference as lref
import sightline_reference as sref  # noqa: F401  (the restatement this one is held against at m = 1)


def cone_axis(i, s, m, N):
    """(first index as int64, f, g) [B, n_ap] of one axis: ``i`` [n_ap] pixel indices, ``s`` and ``m`` [B, 1]."""
    ctr = 0.5 * (N - 1)
    s0 = np.floor(s)
    r = s - s0
    k = m - 1.0
    e = k * (i[None, :] - ctr)
    q = e + r
    q0 = np.floor(q)
    f = q - q0
    g = 1.0 - f
    return i[None, :] + s0.astype(np.int64) + q0.astype(np.int64), f, g


def cone_layer(screen, geom, ap_index, N):
    """v [B, n_ap]: the source's logical screens ``screen`` [B, N_l, N_l] read at (c + ctr + m (iy - ctr) + sy, c + ctr + m (ix - ctr) + sx),
    c = (N_l - N) / 2, for the aperture pixels (iy, ix) = divmod(ap_index, N); ``geom`` [B, 3] = (sx, sy, m).
        v = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))
    Indices modulo N_l."""
    screen = np.asarray(screen, dtype=np.float64)
    geom = np.asarray(geom, dtype=np.float64)
    n = screen.shape[-1]
    assert n >= N and (n - N) % 2 == 0
    c = (n - N) // 2
    iy, ix = np.divmod(np.asarray(ap_index, dtype=np.int64), N)
    sx, sy, m = geom[:, 0:1], geom[:, 1:2], geom[:, 2:3]
    y0, fy, gy = cone_axis(iy, sy, m, N)
    x0, fx, gx = cone_axis(ix, sx, m, N)
    py, px = (c + y0) % n, (c + x0) % n
    py1, px1 = (py + 1) % n, (px + 1) % n
    b = np.arange(screen.shape[0])[:, None]
    v00, v01, v10, v11 = screen[b, py, px], screen[b, py, px1], screen[b, py1, px], screen[b, py1, px1]
    top = (gx * v00) + (fx * v01)
    bottom = (gx * v10) + (fx * v11)
    return (gy * top) + (fy * bottom)


def cone_sum(sources, geometry, ap_index, N, coeff=None, basis=None):
    """s [B, n_ap]: v_0 + v_1 + ... in source order (layers, then mirrors' surfaces), then s = s + coeff[b][k] basis[k][p] in term order.
    ``sources``: arrays [B, N_l, N_l]; ``geometry`` [S, B, 3]."""
    s = None
    for screen, geom in zip(sources, geometry):
        v = cone_layer(screen, geom, ap_index, N)
        s = v if s is None else s + v
    if coeff is not None:
        coeff, basis = np.asarray(coeff, dtype=np.float64), np.asarray(basis, dtype=np.float64)
        for k in range(basis.shape[0]):
            s = s + (coeff[:, k:k + 1] * basis[k][None, :])
    return s


def install(sources, geometry, ap_index, N, wavelength_wfs, coeff=None, basis=None):
    """What the call leaves in a front of B envs: dict(s, mean, psi64, rev, tiles) as ``sightline_reference.install``."""
    s = cone_sum(sources, geometry, ap_index, N, coeff, basis)
    B, n_ap = s.shape
    mean = dref.mean_in_fixed_order(s)
    psi64 = s - mean[:, None]
    rev = (psi64 * (1.0 / (2.0 * np.pi * wavelength_wfs))).astype(np.float32)
    n_ptiles = (n_ap + 31) // 32
    tiles = np.zeros((B + 63) // 64 * 2 * n_ptiles * 1024, dtype=np.float32)
    tiles[lref.tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)] = rev
    return dict(s=s, mean=mean, psi64=psi64, rev=rev, tiles=tiles)


def check(geometry, sizes, N):
    """True when the header's checks pass: finite, 0 < m <= 1, |s| + (1 - m) (N - 1) / 2 <= c_l - 1 (0 when c_l = 0)."""
    g = np.asarray(geometry, dtype=np.float64)
    if not np.all(np.isfinite(g)) or np.any(g[:, :, 2] <= 0) or np.any(g[:, :, 2] > 1):
        return False
    ctr = 0.5 * (N - 1)
    for l, n in enumerate(sizes):
        limit = max((n - N) // 2 - 1, 0)
        if np.any(np.abs(g[l, :, :2]) + ((1.0 - g[l, :, 2:3]) * ctr) > limit):
            return False
    return True
