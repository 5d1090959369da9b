"""Host restatement of the modal telemetry (aog_telemetry_*, csrc/k_telemetry.h) in numpy: the ring, Welch's PSD as a dense DFT, the
rejection |R_k(g)|^2 from its definition, the cost J and its first minimiser.  Every function takes the dtype it computes in: np.float64
is the reference, np.longdouble the yardstick of the reference's own rounding (its envelope)."""
import numpy as np


def pi(dtype):
    return 4 * np.arctan(np.ones((), dtype=dtype))


def complex_of(dtype):
    return np.clongdouble if dtype == np.longdouble else np.complex128


class RingReference:
    """B rings [T, A] float64; sample number c in row c mod T; a row with a non-finite value is skipped and counted."""

    def __init__(self, B, A, T):
        self.B, self.A, self.T = B, A, T
        self.hist = np.zeros((B, T, A))
        self.count = np.zeros(B, dtype=np.int64)
        self.skipped = np.zeros(B, dtype=np.int64)

    def push(self, y, mask=None):
        y = np.asarray(y, dtype=np.float64)
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            if not np.all(np.isfinite(y[b])):
                self.skipped[b] += 1
                continue
            self.hist[b, self.count[b] % self.T] = y[b]
            self.count[b] += 1

    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.hist[b] = 0.0
                self.count[b] = self.skipped[b] = 0

    def series(self, b):
        """What the ring of env b holds, oldest first: [min(count, T), A]."""
        c, T = int(self.count[b]), self.T
        n = min(c, T)
        return self.hist[b, [(c - n + i) % T for i in range(n)]]


def hann(S, dtype=np.float64):
    n = np.arange(S).astype(dtype)
    return (1 - np.cos(2 * pi(dtype) * n / S)) / 2


def dft_tables(S, dtype=np.float64):
    """cos and sin of 2 pi k n / S for k = 0 .. S/2 (the angle reduced exactly: k n mod S)."""
    q = (np.arange(S // 2 + 1)[:, None] * np.arange(S)[None, :]) % S
    ang = 2 * pi(dtype) * q.astype(dtype) / S
    return np.cos(ang), np.sin(ang)


def welch_psd(x, S, dtype=np.float64):
    """x [n, A], oldest first -> (Phi [A, S/2+1], segments).  NaN and 0 when n < S."""
    x = np.asarray(x).astype(dtype)
    n, A = x.shape
    if n < S:
        return np.full((A, S // 2 + 1), np.nan, dtype=dtype), 0
    H = S // 2
    nseg = (n - S) // H + 1
    w = hann(S, dtype)
    c, s = dft_tables(S, dtype)
    acc = np.zeros((S // 2 + 1, A), dtype=dtype)
    first = n - ((nseg - 1) * H + S)
    for i in range(nseg):   # oldest first; the last segment ends at the newest sample
        seg = x[first + i * H:first + i * H + S]
        yw = (seg - seg.mean(axis=0)) * w[:, None]
        re, im = c @ yw, -(s @ yw)
        acc = acc + (re * re + im * im)
    mk = np.full(S // 2 + 1, 2, dtype=dtype)
    mk[0] = mk[-1] = 1
    phi = mk[:, None] * (acc / nseg) / (S * np.sum(w * w))
    return phi.T.copy(), nseg


def rejection(S, delay, grid, dtype=np.float64):
    """|R_k(g)|^2 [G, S/2] for k = 1 .. S/2, from R = 1 / (1 + g z^-d / (1 - z^-1)), z = exp(2 pi i k / S)."""
    ct = complex_of(dtype)
    k = np.arange(1, S // 2 + 1)
    th = 2 * pi(dtype) * k.astype(dtype) / S
    thd = 2 * pi(dtype) * ((k * delay) % S).astype(dtype) / S
    zi = (np.cos(th) - 1j * np.sin(th)).astype(ct)        # z^-1
    zd = (np.cos(thd) - 1j * np.sin(thd)).astype(ct)      # z^-d
    g = np.asarray(grid).astype(dtype)[:, None]
    R = 1 / (1 + g * zd[None, :] / (1 - zi[None, :]))
    return (R.real * R.real + R.imag * R.imag).astype(dtype)


def costs(phi, r2):
    """J [A, G] = sum_{k=1}^{S/2} |R_k(g)|^2 Phi[k]."""
    return phi[:, 1:] @ r2.T


def first_minimiser(J):
    """Index of the first minimum along the last axis (grid order)."""
    return np.argmin(J, axis=-1)


def optimise(x, S, delay, grid, dtype=np.float64):
    """x [n, A] -> (gain [A], cost [A], J [A, G], Phi [A, S/2+1], segments)."""
    phi, nseg = welch_psd(x, S, dtype)
    grid = np.asarray(grid, dtype=np.float64)
    if nseg == 0:
        nan = np.full(phi.shape[0], np.nan)
        return nan, nan.copy(), np.full((phi.shape[0], len(grid)), np.nan), phi, 0
    J = costs(phi, rejection(S, delay, grid, dtype))
    i = first_minimiser(J)
    return grid[i], J[np.arange(J.shape[0]), i], J, phi, nseg


def row_error(a, b):
    """max |a - b| per row as a fraction of the row's largest |b|  (rows along the last axis)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return np.asarray(np.abs(a - b).max(axis=-1) / np.abs(b).max(axis=-1), dtype=np.float64)


def ar1_modes(seed, n, A, pole, drive, noise, mean=0.0):
    """n samples of A independent AR(1) modes x_t = pole x_{t-1} + drive e_t, plus white measurement noise and a mean (all per mode)."""
    rng = np.random.RandomState(seed)
    pole, drive, noise, mean = (np.broadcast_to(np.asarray(v, dtype=np.float64), (A,)) for v in (pole, drive, noise, mean))
    x = np.zeros((n + 64, A))
    e = rng.randn(n + 64, A)
    for t in range(1, n + 64):
        x[t] = pole * x[t - 1] + drive * e[t]
    return x[64:] + noise * rng.randn(n, A) + mean
