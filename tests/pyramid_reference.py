"""Host restatement of the modulated pyramid wavefront sensor ("Pyramid sensor"; include/aogym.h), float64 numpy, written
from the model and not from the package's ``pyramid_host``: frames, slopes, calibration, the integrator loop and the photon stream.

Lengths are in pupil pixels centred on the pupil (pixel y at y - (N - 1) / 2), focal positions in lambda_wfs / D.  Quadrant index
2 (k_y > 0) + (k_x > 0).  Here every quadrant's back transform runs over its own w_q x w_q block of the focal field (the package
multiplies the whole window by matrices that are zero outside the block)."""
import numpy as np

import detector_reference as det

FRAME_XOR = 0x9F2A31D     # word 3 of the photon stream's Philox counter is (frame >> 32) ^ FRAME_XOR; word 0 the bare pixel index


class Sensor:
    def __init__(self, n_pupil, ap_index, samples, q=2, pixels=32, n_mod=8, r_mod=3.0):
        self.N, self.wq, self.q, self.ns, self.n_mod, self.r_mod = int(n_pupil), int(samples), int(q), int(pixels), int(n_mod), float(r_mod)
        self.ap_index = np.asarray(ap_index)
        self.n_ap = int(self.ap_index.size)
        N, wq, ns = self.N, self.wq, self.ns
        w = 2 * wq
        self.k = np.array([(i + 0.5 - w / 2) / self.q for i in range(w)])
        ang = np.array([2 * np.pi * (j + 0.5) / self.n_mod for j in range(self.n_mod)])
        self.kappa_x, self.kappa_y = self.r_mod * np.cos(ang), self.r_mod * np.sin(ang)
        y = np.arange(N) - (N - 1) / 2
        self.y = y
        norm = 1.0 / np.sqrt(self.n_ap)
        # forward: m1_j [w, N] over (k_y, y), m2_j [N, w] over (x, k_x)
        self.m1 = [np.exp(-2j * np.pi * (self.k[:, None] - ky) * y[None, :] / N) * norm for ky in self.kappa_y]
        self.m2 = [np.exp(-2j * np.pi * y[:, None] * (self.k[None, :] - kx) / N) * norm for kx in self.kappa_x]
        # back: detector pixel centres, b [n_s, w]
        self.yd = (np.arange(ns) + 0.5 - ns / 2) * (N / ns)
        self.b = np.exp(2j * np.pi * self.yd[:, None] * self.k[None, :] / N) * np.sqrt(1.0 / self.q)
        self.valid_mask = self.yd[:, None] ** 2 + self.yd[None, :] ** 2 <= (N / 2) ** 2
        self.valid = np.flatnonzero(self.valid_mask.ravel())

    # -- field and frames ---------------------------------------------------------------------------
    def field(self, u_rev):
        """E [N, N]: exp(2 pi i u) on the aperture pixels (u_rev [n_ap] in revolutions), 0 elsewhere."""
        E = np.zeros(self.N * self.N, dtype=np.complex128)
        E[self.ap_index] = np.exp(2j * np.pi * np.asarray(u_rev, dtype=np.float64))
        return E.reshape(self.N, self.N)

    def focal(self, E, j):
        return self.m1[j] @ E @ self.m2[j]

    def frame(self, u_rev):
        """[4, n_s, n_s] float64, noise-free."""
        E = self.field(u_rev)
        wq = self.wq
        halves = (slice(0, wq), slice(wq, 2 * wq))
        acc = np.zeros((4, self.ns, self.ns))
        for j in range(self.n_mod):
            F = self.focal(E, j)
            for sy in range(2):
                for sx in range(2):
                    G = self.b[:, halves[sy]] @ F[halves[sy], halves[sx]] @ self.b[:, halves[sx]].T
                    acc[2 * sy + sx] += G.real ** 2 + G.imag ** 2
        return acc / self.n_mod

    def slopes_of(self, frame):
        """[2 n_valid]: s_x over the valid pixels, then s_y."""
        I = np.asarray(frame, dtype=np.float64).reshape(4, -1)[:, self.valid]
        ibar = I.sum(axis=0).mean()
        return np.concatenate([(I[1] + I[3] - I[0] - I[2]) / ibar, (I[2] + I[3] - I[0] - I[1]) / ibar])

    def slopes(self, u_rev):
        return self.slopes_of(self.frame(u_rev))

    # -- photon noise -------------------------------------------------------------------------------
    def photon_words(self, env_ids, seed, frame_index):
        """uint32 [len(env_ids), 4 n_s^2, 4]: the Philox words of every (env, pixel) of a sensor call."""
        return det.detector_words(4 * self.ns * self.ns, env_ids, seed, frame_index, tag=0, frame_xor=FRAME_XOR)

    def noisy(self, clean, photons, env_ids, seed, frame_index):
        """clean [B, 4, n_s, n_s] (the frame BEFORE noise, as the device formed it) -> (noisy frame, undecidable), same shape:
        large_poisson(photons x clean) / photons from word 0 (uniform / radius) and word 1 (angle)."""
        c = np.asarray(clean, dtype=np.float64)
        lam = float(photons) * c.reshape(c.shape[0], -1)
        n, und = det.counts(lam, self.photon_words(env_ids, seed, frame_index))
        return (n / float(photons)).reshape(c.shape), und.reshape(c.shape)


def phase_rev(screen, modes, actuators, ap_index, wavelength_wfs):
    """u [n_ap] in revolutions of lambda_wfs: the achromatic screen (phase x lambda) on the aperture plus the mirror (surface = modes a,
    metres; the path doubles on reflection)."""
    psi = np.asarray(screen, dtype=np.float64).ravel()[np.asarray(ap_index)] / (2 * np.pi * wavelength_wfs)
    return psi + 2.0 * (np.asarray(modes, dtype=np.float64) @ np.asarray(actuators, dtype=np.float64)) / wavelength_wfs


def inverse_tikhonov(response, rcond):
    U, S, Vt = np.linalg.svd(response, full_matrices=False)
    return (Vt.T * (S / (S ** 2 + (rcond * S.max()) ** 2))) @ U.T


def calibrate(sensor, modes, wavelength_wfs, poke, rcond):
    """(R [A, 2 n_valid], s_ref [2 n_valid], response [2 n_valid, A]): push-pull pokes of every mode on a flat wavefront."""
    A = modes.shape[1]
    flat = np.zeros(sensor.N * sensor.N)
    s_ref = sensor.slopes(phase_rev(flat, modes, np.zeros(A), sensor.ap_index, wavelength_wfs))
    resp = np.empty((s_ref.size, A))
    for k in range(A):
        a = np.zeros(A)
        a[k] = poke
        sp = sensor.slopes(phase_rev(flat, modes, a, sensor.ap_index, wavelength_wfs))
        sm = sensor.slopes(phase_rev(flat, modes, -a, sensor.ap_index, wavelength_wfs))
        resp[:, k] = (sp - sm) / (2 * poke)
    return inverse_tikhonov(resp, rcond), s_ref, resp


def integrate(sensor, screen, modes, wavelength_wfs, R, s_ref, gain, steps, a0=None):
    """The integrator on a static screen: a <- a - gain R (s(a) - s_ref).  Returns (actuators [steps + 1, A], slopes [steps, 2 n_valid])."""
    a = np.zeros(modes.shape[1]) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    acts, sl = [a.copy()], []
    for _ in range(steps):
        s = sensor.slopes(phase_rev(screen, modes, a, sensor.ap_index, wavelength_wfs))
        a = a - gain * (R @ (s - s_ref))
        acts.append(a.copy())
        sl.append(s)
    return np.array(acts), np.array(sl)


def residual_rms(screen, modes, actuators, ap_index, wavelength_wfs):
    """RMS of the residual phase over the aperture in radians at lambda_wfs (piston removed)."""
    u = 2 * np.pi * phase_rev(screen, modes, actuators, ap_index, wavelength_wfs)
    return float(np.std(u))


def literal_frame(sensor, u_rev, isolate=False):
    """The literal pyramid at n_mod = 1, r_mod = 0, n_s = N: zero-padded FFT of the pupil onto the whole period of the focal plane
    (M = q N samples per axis at the sensor's k grid extended to the period), the four-facet phase mask that carries quadrant (s_y, s_x)
    to an image centred at (s_y, s_x) N / 2, the inverse FFT, and the four N x N images cut out of the 2 N x 2 N output (q = 2).
    [4, N, N] float64 in the model's normalisation.  ``isolate``: every image from its own facet alone (the other three quadrants of the
    focal plane blocked), which takes the interference between the four beams out and leaves the model's own statement."""
    N, q = sensor.N, sensor.q
    assert q == 2 and sensor.ns == N and sensor.n_mod == 1 and sensor.r_mod == 0.0
    M = q * N
    E = sensor.field(u_rev)
    m = np.arange(M)
    a, b = 0.5 - M / 2, -(N - 1) / 2           # k_m = (m + a) / q, pupil pixel y at y + b
    # F[m] = sum_y E[y] exp(-2 pi i (m + a) (y + b) / M) / sqrt(n_ap), as a padded FFT with phase ramps before and after
    pre = np.exp(-2j * np.pi * a * (np.arange(N) + b) / M)
    post = np.exp(-2j * np.pi * m * b / M)
    pad = np.zeros((M, M), dtype=np.complex128)
    pad[:N, :N] = E * pre[:, None] * pre[None, :]
    F = np.fft.fft2(pad) * post[:, None] * post[None, :] / sensor.n_ap
    k = (m + a) / q
    facet = np.exp(-2j * np.pi * np.abs(k) * (N / 2) / N)       # shifts the image of the half k > 0 by +N/2, of k < 0 by -N/2
    F = F * facet[:, None] * facet[None, :]
    # G[Y] = (1 / q) sum_m F[m] exp(+2 pi i k_m Yc / N), Yc = Y - (M - 1) / 2, as an inverse FFT with ramps
    Yc = m - (M - 1) / 2
    pre2 = np.exp(2j * np.pi * m * (-(M - 1) / 2) / M)
    post2 = np.exp(2j * np.pi * a * Yc / M)
    def images(Fm):
        G = np.fft.ifft2(Fm * pre2[:, None] * pre2[None, :]) * (M * M) * post2[:, None] * post2[None, :] / q
        return G.real ** 2 + G.imag ** 2

    cut = lambda I, sy, sx: I[sy * N:(sy + 1) * N, sx * N:(sx + 1) * N]
    if not isolate:
        I = images(F)
        return np.array([cut(I, sy, sx) for sy in range(2) for sx in range(2)])
    # one facet at a time: only the quadrant (s_y, s_x) of the focal plane is kept, so no other facet's light reaches its image
    side = (k < 0, k > 0)
    return np.array([cut(images(F * side[sy][:, None] * side[sx][None, :]), sy, sx) for sy in range(2) for sx in range(2)])
