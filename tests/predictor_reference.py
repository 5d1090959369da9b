"""A numpy restatement of the recursive-least-squares predictor of ``aog_predictor_update`` (include/aogym.h), for float64 and for
``np.longdouble``: the same operation order per element in both, every sum a plain ascending one (``np.cumsum``'s last entry: it adds one element after the other).

    c = count as the call finds it, x_ the history (newest measurement first, divided by scale)
    c >= order:  e = y / scale - W' x_;  g = P x_;  d = lam + x_' g;  W[i][j] += (g[i] / d) e[j];  P[i][j] = (P[i][j] - (g[i] g[j]) / d) / lam
    push y / scale, count = c + 1
    c >= order:  pred = scale W' x (new W, new x), innov = scale e;  otherwise pred = y (the same bits), innov = 0
    a row of y with a non-finite value: nothing changes, pred = y, innov = 0, skipped += 1

``device_sums=True`` keeps every operation but adds the dot products in the order the HIP kernel does (csrc/k_predictor.h: the rows in
blocks of one wave, the blocks in wave order; x' g over strides of 64 and a butterfly) — float64 arithmetic that differs from the plain
form by summation order alone, which is all the device is allowed to differ by."""
import numpy as np


def device_geometry(n, A):
    """(waves, rows per wave) of the kernel variant that serves (n, A)."""
    if n <= 64:
        return 4, 16
    if n <= 128:
        return 8, 16
    return 8, (n + 7) // 8


class RLSReference:
    def __init__(self, batch, act_dim, order, forgetting, p0, scale, dtype=np.float64, device_sums=False):
        self.B, self.A, self.p, self.n = int(batch), int(act_dim), int(order), int(act_dim) * int(order)
        self.dt = dtype
        self.lam, self.p0, self.scale = dtype(forgetting), dtype(p0), dtype(scale)
        self.device_sums = bool(device_sums)
        self.reset()

    def reset(self, mask=None):
        B, A, n, dt = self.B, self.A, self.n, self.dt
        if mask is None:
            self.W = np.zeros((B, n, A), dt)
            self.P = np.zeros((B, n, n), dt)
            self.hist = np.zeros((B, n), dt)
            self.count = np.zeros(B, np.int64)
            self.skipped = np.zeros(B, np.int64)
            mask = np.ones(B, bool)
        mask = np.asarray(mask, bool)
        self.W[mask] = 0
        self.P[mask] = 0
        for i in range(A):
            self.W[mask, i, i] = 1
        for i in range(n):
            self.P[mask, i, i] = self.p0
        self.hist[mask] = 0
        self.count[mask] = 0
        self.skipped[mask] = 0

    # --- the dot products: rows [lo, hi) added in ascending order
    def _colsum(self, M, x, lo, hi):
        if hi <= lo:
            return np.zeros((M.shape[0], M.shape[2]), self.dt)
        return np.cumsum(M[:, lo:hi, :] * x[:, lo:hi, None], axis=1)[:, -1, :]   # (cumsum adds one after the other)

    def _mat_t_vec(self, M, x):
        """sum_i M[i][j] x[i] for every j."""
        n = self.n
        if not self.device_sums:
            return self._colsum(M, x, 0, n)
        nw, rpw = device_geometry(n, self.A)
        tot = None
        for w in range(nw):
            part = self._colsum(M, x, min(w * rpw, n), min((w + 1) * rpw, n))
            tot = part if tot is None else tot + part
        return tot

    def _dot(self, x, g):
        n = self.n
        if not self.device_sums:
            return np.cumsum(x * g, axis=1)[:, -1]
        lanes = np.zeros((x.shape[0], 64), self.dt)
        for i0 in range(0, n, 64):
            m = min(64, n - i0)
            lanes[:, :m] = lanes[:, :m] + x[:, i0:i0 + m] * g[:, i0:i0 + m]
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, np.arange(64) ^ off]
        return lanes[:, 0]

    def update(self, y, mask=None):
        """y [B, A] float64 -> (pred, innov) in the reference's dtype; rows the mask leaves out come back as NaN (they are not written)."""
        B, A, n, dt = self.B, self.A, self.n, self.dt
        y = np.asarray(y, np.float64)
        sel = np.ones(B, bool) if mask is None else np.asarray(mask, bool).copy()
        pred = np.full((B, A), np.nan, dt)
        innov = np.full((B, A), np.nan, dt)
        bad = sel & ~np.isfinite(y).all(axis=1)
        pred[bad] = y[bad]
        innov[bad] = 0
        self.skipped[bad] += 1
        sel &= ~bad
        have = sel & (self.count >= self.p)
        warm = sel & ~have
        z = y.astype(dt) / self.scale
        xnew = np.concatenate([z, self.hist[:, :n - A]], axis=1)
        pred[warm] = y[warm]
        innov[warm] = 0
        if have.any():
            h = np.nonzero(have)[0]
            W, P, x = self.W[h], self.P[h], self.hist[h]
            # (P x through P's columns: P is symmetric bit for bit, so this is the row sum, element for element)
            e = z[h] - self._mat_t_vec(W, x)
            g = self._mat_t_vec(P, x) if self.device_sums else self._row_sums(P, x)
            d = self.lam + self._dot(x, g)
            k = g / d[:, None]
            W = W + k[:, :, None] * e[:, None, :]
            P = (P - (g[:, :, None] * g[:, None, :]) / d[:, None, None])
            if self.lam != 1:
                P = P / self.lam
            self.W[h], self.P[h] = W, P
            pred[h] = self.scale * self._mat_t_vec(W, xnew[h])
            innov[h] = self.scale * e
        self.hist[sel] = xnew[sel]
        self.count[sel] += 1
        return pred, innov

    def _row_sums(self, P, x):
        return np.cumsum(P * x[:, None, :], axis=2)[:, :, -1]


def var1_sequence(seed, T, B, A, amplitude=1e-7, rho=0.95, noise=0.05):
    """A seeded stationary VAR(1) process plus white noise, [T, B, A] float64 of about ``amplitude``: s_{t+1} = rho Q s_t + sqrt(1 - rho^2) w_t
    with Q a fixed orthogonal matrix per env, y_t = amplitude (s_t + noise v_t)."""
    rng = np.random.RandomState(seed)
    Q = np.stack([np.linalg.qr(rng.randn(A, A))[0] for _ in range(B)])
    s = rng.randn(B, A)
    out = np.empty((T, B, A))
    for t in range(T):
        out[t] = amplitude * (s + noise * rng.randn(B, A))
        s = rho * np.einsum("bij,bj->bi", Q, s) + np.sqrt(1.0 - rho * rho) * rng.randn(B, A)
    return out


def run(ref, ys, masks=None):
    """Feed ys [T, B, A]; returns (pred [T, B, A], innov [T, B, A])."""
    preds, innovs = [], []
    for t, y in enumerate(ys):
        p, i = ref.update(y, None if masks is None else masks[t])
        preds.append(p)
        innovs.append(i)
    return np.stack(preds), np.stack(innovs)


def rel_diff(a, b):
    """max |a - b| relative to max |b| (finite entries; both must be non-finite in the same places)."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a))
    if not fin.any():
        return 0.0
    return float(np.abs(a[fin] - b[fin]).max() / np.abs(b[fin]).max())
