"""Host restatement of aog_sh_gradient (include/aogym_shack_gradient.h; DESIGN.md "Shack-Hartmann chain: gradient"), float64 numpy, on top
of ``sh_host.ShackHartmannHost``: the clean image and slopes of one env, their vector-Jacobian product with respect to the sensor mirror's
actuators, and the full Jacobian by columns.

Forward, per env (a: actuators in metres, M: modes on the aperture pixels, phi_atm: the screen's phase at lambda_wfs on them):
    f = amp exp(i (phi_atm + 2 k M a)),  e = f / mag * mla_phase,  v = crop_N(IFFT2(FFT2(pad_2N(e)) H)),  I = |v|^2 image_scale
    per selected lenslet s, with I' = I + 1e-10:  F_s = sum I',  c_s = sum I' (x, y) / F_s;  slopes = c - centres - slopes_ref
Backward of L = sum g_image I + sum g_slopes slopes:
    g_I = g_image + [g_sx (x - c_x) + g_sy (y - c_y)] / F on the lenslets' pixels,  g_v = image_scale g_I v,
    g_e = crop_N(IFFT2(FFT2(pad_2N(g_v)) conj(H))),  g_f = g_e conj(mla_phase) / mag,  g_phi = 2 Im(conj(f) g_f),  grad = 2 k M' g_phi"""
import numpy as np


def propagate(sh, e, conj=False):
    """crop_N(IFFT2(FFT2(pad_2N(e)) H)) of an [N, N] field; ``conj=True``: with conj(H), which is this operator's adjoint."""
    N = sh.N
    pad = np.zeros((2 * N, 2 * N), dtype=complex)
    pad[:N, :N] = e
    return np.fft.ifft2(np.fft.fft2(pad) * (np.conj(sh.transfer) if conj else sh.transfer))[:N, :N]


def atmosphere_phase(sh, screen, wavelength_wfs):
    """phi_atm [n_ap]: the achromatic screen (phase x lambda, [N, N]) at the sensing wavelength on the aperture pixels."""
    return np.asarray(screen, dtype=np.float64).ravel()[sh.ap_index] / wavelength_wfs


class Point:
    """Everything the forward pass leaves at one point of evaluation."""

    def __init__(self, sh, phi_atm, actuators, amp, dt):
        N = sh.N
        self.sh, self.scale = sh, sh.pitch ** 2 * dt
        self.f = amp * np.exp(1j * (np.asarray(phi_atm, dtype=np.float64) + 2 * sh.k_wfs * (sh.modes @ np.asarray(actuators, dtype=np.float64))))
        field = np.zeros(N * N, dtype=complex)
        field[sh.ap_index] = self.f
        self.v = propagate(sh, (field / sh.mag * sh.mla_phase).reshape(N, N))
        self.image = (np.abs(self.v) ** 2).ravel() * self.scale
        self.sel = sh.sub_slot >= 0
        self.slot = sh.sub_slot[self.sel]
        self.xs = np.tile(sh.x_det, N)[self.sel]
        self.ys = np.repeat(sh.x_det, N)[self.sel]
        w = self.image[self.sel] + 1e-10                                  # estimate([image + 1e-10]) (AO_env.py:277)
        self.flux = np.bincount(self.slot, weights=w, minlength=sh.n_sub)
        self.cx = np.bincount(self.slot, weights=w * self.xs, minlength=sh.n_sub) / self.flux
        self.cy = np.bincount(self.slot, weights=w * self.ys, minlength=sh.n_sub) / self.flux
        self.slopes = np.concatenate([self.cx - sh.centres[:, 0], self.cy - sh.centres[:, 1]]) - sh.slopes_ref

    def image_cotangent(self, g_image=None, g_slopes=None):
        """g_I [N*N]: the cotangent on the image, the slopes cotangent pulled back through the centroids."""
        sh = self.sh
        g = np.zeros(sh.N ** 2) if g_image is None else np.array(g_image, dtype=np.float64).ravel()
        if g_slopes is not None:
            gs = np.asarray(g_slopes, dtype=np.float64)
            gx, gy = gs[:sh.n_sub], gs[sh.n_sub:]
            s = self.slot
            g[self.sel] += (gx[s] * (self.xs - self.cx[s]) + gy[s] * (self.ys - self.cy[s])) / self.flux[s]
        return g

    def vjp(self, g_image=None, g_slopes=None):
        """grad [A] per metre of surface."""
        sh = self.sh
        g_v = self.scale * self.image_cotangent(g_image, g_slopes).reshape(sh.N, sh.N) * self.v
        g_f = (propagate(sh, g_v, conj=True).ravel() * np.conj(sh.mla_phase) / sh.mag)[sh.ap_index]
        g_phi = 2.0 * np.imag(np.conj(self.f) * g_f)
        return 2 * sh.k_wfs * (sh.modes.T @ g_phi)

    def jacobian(self):
        """(J_image [N*N, A], J_slopes [2 n_sub, A]): column k by pushing the tangent of actuator k forward."""
        sh = self.sh
        N, A = sh.N, sh.modes.shape[1]
        Ji, Js = np.empty((N * N, A)), np.empty((2 * sh.n_sub, A))
        s = self.slot
        for k in range(A):
            df = np.zeros(N * N, dtype=complex)
            df[sh.ap_index] = 2j * sh.k_wfs * sh.modes[:, k] * self.f
            dv = propagate(sh, (df / sh.mag * sh.mla_phase).reshape(N, N))
            dI = (2.0 * self.scale * np.real(np.conj(self.v) * dv)).ravel()
            Ji[:, k] = dI
            w = dI[self.sel]
            Js[:sh.n_sub, k] = np.bincount(s, weights=w * (self.xs - self.cx[s]), minlength=sh.n_sub) / self.flux
            Js[sh.n_sub:, k] = np.bincount(s, weights=w * (self.ys - self.cy[s]), minlength=sh.n_sub) / self.flux
        return Ji, Js


def clean(sh, phi_atm, actuators, amp, dt):
    """(image [N*N], slopes [2 n_sub]) at ``actuators``."""
    p = Point(sh, phi_atm, actuators, amp, dt)
    return p.image, p.slopes


def grad(sh, phi_atm, actuators, amp, dt, g_image=None, g_slopes=None):
    """(grad [A], image, slopes): what aog_sh_gradient returns for one env."""
    p = Point(sh, phi_atm, actuators, amp, dt)
    return p.vjp(g_image, g_slopes), p.image, p.slopes
