"""Host restatement of the modal disturbance (include/aogym_disturbance.h) in numpy float64, written from the header's text: the
generator's recursion fed with recorded normals, and the disturbed layer sum on top of ``layered_reference``.  numpy's float64 ``*``, ``+``
and ``sqrt`` are single correctly rounded operations and nothing here is fused, so the device must match these bit for bit."""
import numpy as np

import layered_reference as lref

PARAMETERS = ("a1", "a2", "b", "sigma", "rho1", "offset")


class Generator:
    """State x, x_prev [B, K] and the call counter of one handle; ``params``: dict of [B, K] arrays (a1, a2, b, sigma, rho1, offset)."""

    def __init__(self, params):
        self.p = {k: np.asarray(params[k], dtype=np.float64) for k in PARAMETERS}
        self.x = np.zeros_like(self.p["a1"])
        self.x_prev = np.zeros_like(self.x)
        self.counter = 0

    def _sel(self, mask):
        B = self.x.shape[0]
        return np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)

    def reset(self, normals, mask=None):
        """normals [B, K, 2] = (n0, n1): x_prev = sigma n0, x = sigma (rho1 n0 + sqrt(1 - rho1 rho1) n1) for the selected envs."""
        sel, p = self._sel(mask), self.p
        n0, n1 = normals[..., 0], normals[..., 1]
        root = np.sqrt(1.0 + -(p["rho1"] * p["rho1"]))
        x_prev = p["sigma"] * n0
        x = p["sigma"] * ((p["rho1"] * n0) + (root * n1))
        self.x_prev[sel], self.x[sel] = x_prev[sel], x[sel]
        self.counter += 1

    def advance(self, normals, mask=None):
        """normals [B, K]: x_new = (a1 x + a2 x_prev) + b n; returns coeff = offset + x (x_new for the selected envs)."""
        sel, p = self._sel(mask), self.p
        x_new = ((p["a1"] * self.x) + (p["a2"] * self.x_prev)) + (p["b"] * normals)
        self.x_prev[sel] = self.x[sel]
        self.x[sel] = x_new[sel]
        self.counter += 1
        return self.coefficients()

    def coefficients(self):
        return self.p["offset"] + self.x

    def blob(self):
        """The checkpoint blob: x, x_prev, counter."""
        return np.concatenate([self.x.ravel().view(np.uint8), self.x_prev.ravel().view(np.uint8), np.array([self.counter], dtype=np.uint64).view(np.uint8)])


def disturbed_sum(masters, origins, ap_index, N, coeff, basis):
    """s [B, n_ap]: the layer sum, then s = s + coeff[b][k] basis[k][p] in term order (product rounded, then the sum)."""
    s = lref.layer_sum(masters, origins, ap_index, N)
    coeff, basis = np.asarray(coeff, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    for k in range(basis.shape[0]):
        s = s + (coeff[:, k:k + 1] * basis[k][None, :])
    return s


def mean_in_fixed_order(s):
    """The aperture mean of s [B, n_ap] in the fixed order the header states for pass 1: 256 partial sums, partial t = s[t] + s[t + 256] +
    s[t + 512] + ... ascending from 0; each run of 64 partials folded in six halving steps (v[i] += v[i + off], off = 32, 16, 8, 4, 2, 1);
    the four results added in order from 0; divided by n_ap."""
    B, n = s.shape
    a = np.concatenate([s, np.zeros((B, (-n) % 256))], axis=1).reshape(B, -1, 256)
    acc = np.zeros((B, 256))
    for j in range(a.shape[1]):
        acc = acc + a[:, j]
    v = acc.reshape(B, 4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :, :off] = v[:, :, :off] + v[:, :, off:2 * off]
    total = np.zeros(B)
    for w in range(4):
        total = total + v[:, w, 0]
    return total / n


def install(masters, origins, ap_index, N, wavelength_wfs, coeff, basis):
    """``layered_reference.install`` of the disturbed sum, with the mean summed in the fixed order: dict(s, mean, psi64, rev, tiles)."""
    s = disturbed_sum(masters, origins, ap_index, N, coeff, basis)
    B, n_ap = s.shape
    mean = mean_in_fixed_order(s)
    psi64 = s - mean[:, None]
    rev = (psi64 * (1.0 / (2.0 * np.pi * wavelength_wfs))).astype(np.float32)
    n_ptiles = (n_ap + 31) // 32
    tiles = np.zeros((B + 63) // 64 * 2 * n_ptiles * 1024, dtype=np.float32)
    tiles[lref.tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)] = rev
    return dict(s=s, mean=mean, psi64=psi64, rev=rev, tiles=tiles)


def ar2_variance(a1, a2, b):
    """The stationary variance of x_t = a1 x_{t-1} + a2 x_{t-2} + b n_t from the 2 x 2 Yule-Walker system in (gamma_0, gamma_1):
    gamma_1 = a1 gamma_0 + a2 gamma_1,  gamma_0 = a1 gamma_1 + a2 gamma_2 + b^2 with gamma_2 = a1 gamma_1 + a2 gamma_0."""
    A = np.array([[a1, a2 - 1.0], [1.0 - a2 * a2, -(a1 + a1 * a2)]])
    g0, _ = np.linalg.solve(A, np.array([0.0, b * b]))
    return g0


def ar2_spectrum(a1, a2, b, freqs, delta_t):
    """|b / (1 - a1 z^-1 - a2 z^-2)|^2 at z = exp(2 pi i f dt)."""
    z = np.exp(-2j * np.pi * np.asarray(freqs) * delta_t)
    return np.abs(b / (1.0 - a1 * z - a2 * z * z)) ** 2
