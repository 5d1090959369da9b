"""Host restatement of the scintillation kernels (include/aogym_scintillation.h) in numpy float64: the mirror extension, the filter table
of ``scintillation.rytov_filters`` (the very table the device multiplies by), ``numpy.fft``, the bilinear read of
``sightline_reference.displaced_layer`` and the receiver's sums."""
import numpy as np

import sightline_reference as sref


def mirror_extend(screen):
    """[..., M, M] -> [..., 2 M, 2 M]: ext[y][x] = screen[y < M ? y : 2 M - 1 - y][x < M ? x : 2 M - 1 - x]."""
    s = np.asarray(screen, dtype=np.float64)
    s = np.concatenate([s, s[..., ::-1, :]], axis=-2)
    return np.concatenate([s, s[..., ::-1]], axis=-1)


def filter_layer(screen, table):
    """(S, chi) of logical screens [B, M, M] through ``table`` [2 M, 2 M, 2] (cos, sin): one complex inverse transform of
    (cos + i sin) F ext, cropped to the first M x M pixels.  In the screens' unit."""
    screen = np.asarray(screen, dtype=np.float64)
    M = screen.shape[-1]
    spec = np.fft.fft2(mirror_extend(screen)) * (table[..., 0] + 1j * table[..., 1])
    out = np.fft.ifft2(spec)[..., :M, :M]
    return out.real, out.imag


def filter_periodic(screen, altitude, wavelength, pitch):
    """(S, chi) of a screen taken as periodic on its own grid (no extension): the big-screen side of the edge measurement."""
    screen = np.asarray(screen, dtype=np.float64)
    fy, fx = np.fft.fftfreq(screen.shape[-2], pitch), np.fft.fftfreq(screen.shape[-1], pitch)
    arg = np.pi * wavelength * altitude * (fy[:, None] ** 2 + fx[None, :] ** 2)
    out = np.fft.ifft2(np.fft.fft2(screen) * np.exp(1j * arg))
    return out.real, out.imag


def chi_map(chis, shifts, ap_index, N, wavelength):
    """[B, n_ap] float32: (chi_0 + chi_1 + ... read at ``shifts`` [L, B, 2]) x (1 / lambda), rounded to float32 — what aog_scint_install
    stores.  ``chis``: L arrays [B, M, M]."""
    s = None
    for chi, shift in zip(chis, shifts):
        v = sref.displaced_layer(chi, shift, ap_index, N)
        s = v if s is None else s + v
    return (s * (1.0 / wavelength)).astype(np.float32)


def receive(u, chi, modes):
    """The receiver's dict for residual phases ``u`` [B, n_ap] (revolutions), log-amplitudes ``chi`` [B, n_ap] (nepers) and receive modes
    [K, n_ap] complex, all in float64."""
    u, chi = np.asarray(u, dtype=np.float64), np.asarray(chi, dtype=np.float64)
    a = np.exp(chi)
    field = a * np.exp(2j * np.pi * u)
    c = field @ np.asarray(modes).T
    on_axis = field.sum(axis=1)
    return dict(power=(np.abs(c) ** 2).sum(axis=1), irradiance=(a * a).mean(axis=1), strehl=np.abs(on_axis) ** 2 / a.sum(axis=1) ** 2,
                sigma_chi2=(chi * chi).mean(axis=1) - chi.mean(axis=1) ** 2)
