"""Host restatement of ``aog_install_layer_sum_sightline`` (include/aogym_sightline.h) in numpy float64, written from the header's text:
the bilinear read of every layer's meta-pupil at its own shift, the layer sum, the modal terms, the mean in its fixed order and the
front's two stores.  numpy's float64 ``*``, ``+``, ``-`` and ``floor`` are single correctly rounded operations and nothing here is fused,
so a float64 front must match ``psi64`` bit for bit."""
import numpy as np

import disturbance_reference as dref
import layered_reference as lref


def displaced_layer(screen, shift, ap_index, N):
    """v [B, n_ap]: the layer's logical screens ``screen`` [B, N_l, N_l] read at (iy + c + sy, ix + c + sx), c = (N_l - N) / 2, for the
    aperture pixels (iy, ix) = divmod(ap_index, N); ``shift`` [B, 2] = (sx, sy).
        v = (gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))
    Indices wrap modulo N_l as the ring does (only a shift at the margin's edge, or c = 0, reaches the wrap)."""
    screen = np.asarray(screen, dtype=np.float64)
    shift = np.asarray(shift, dtype=np.float64)
    n = screen.shape[-1]
    assert n >= N and (n - N) % 2 == 0
    c = (n - N) // 2
    iy, ix = np.divmod(np.asarray(ap_index, dtype=np.int64), N)
    sx, sy = shift[:, 0:1], shift[:, 1:2]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    gx, gy = 1.0 - fx, 1.0 - fy
    py = (iy[None, :] + c + y0.astype(np.int64)) % n
    px = (ix[None, :] + c + x0.astype(np.int64)) % n
    py1, px1 = (py + 1) % n, (px + 1) % n
    b = np.arange(screen.shape[0])[:, None]
    v00, v01, v10, v11 = screen[b, py, px], screen[b, py, px1], screen[b, py1, px], screen[b, py1, px1]
    top = (gx * v00) + (fx * v01)
    bottom = (gx * v10) + (fx * v11)
    return (gy * top) + (fy * bottom)


def sightline_sum(screens, shifts, ap_index, N, coeff=None, basis=None):
    """s [B, n_ap]: v_0 + v_1 + ... in layer order, then s = s + coeff[b][k] basis[k][p] in term order (product rounded, then the sum).
    ``screens``: L arrays [B, N_l, N_l]; ``shifts`` [L, B, 2]."""
    s = None
    for screen, shift in zip(screens, shifts):
        v = displaced_layer(screen, shift, ap_index, N)
        s = v if s is None else s + v
    if coeff is not None:
        coeff, basis = np.asarray(coeff, dtype=np.float64), np.asarray(basis, dtype=np.float64)
        for k in range(basis.shape[0]):
            s = s + (coeff[:, k:k + 1] * basis[k][None, :])
    return s


def install(screens, shifts, ap_index, N, wavelength_wfs, coeff=None, basis=None):
    """What the call leaves in a front of B envs: dict(s, mean, psi64, rev, tiles) as ``disturbance_reference.install``."""
    s = sightline_sum(screens, shifts, ap_index, N, coeff, basis)
    B, n_ap = s.shape
    mean = dref.mean_in_fixed_order(s)
    psi64 = s - mean[:, None]
    rev = (psi64 * (1.0 / (2.0 * np.pi * wavelength_wfs))).astype(np.float32)
    n_ptiles = (n_ap + 31) // 32
    tiles = np.zeros((B + 63) // 64 * 2 * n_ptiles * 1024, dtype=np.float32)
    tiles[lref.tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)] = rev
    return dict(s=s, mean=mean, psi64=psi64, rev=rev, tiles=tiles)
