"""The LQG controller of include/aogym_lqg.h restated in numpy float64, operation for operation: the definition csrc/k_lqg.h is held to.

Every array is [B, ..., A]; every ``*`` , ``+`` and ``/`` below is one numpy ufunc call on float64, hence one rounded operation per element,
and the order of the sums is the header's (left to right from the first term).  Nothing here is fused or reassociated: do not "tidy" a
sum into ``np.sum`` or a product into ``@``."""
import numpy as np


def companion(a):
    """A [n, n] of one (env, mode): a [S, 2]."""
    S = a.shape[0]
    out = np.zeros((2 * S, 2 * S))
    for s in range(S):
        out[2 * s, 2 * s], out[2 * s, 2 * s + 1], out[2 * s + 1, 2 * s] = a[s, 0], a[s, 1], 1.0
    return out


class LQGReference:
    """B envs, A modes, S sub-models: the records of an ``aog_lqg`` handle and its four calls."""

    def __init__(self, B, A, S):
        self.B, self.A, self.S, self.n = int(B), int(A), int(S), 2 * int(S)
        B, A, S, n = self.B, self.A, self.S, self.n
        self.a, self.q, self.r = np.zeros((B, S, 2, A)), np.zeros((B, S, A)), np.zeros((B, A))
        self.K, self.c, self.conv, self.solved = np.zeros((B, n, A)), np.zeros((B, n, A)), np.zeros((B, A)), np.zeros((B, A))
        self.xhat, self.command = np.zeros((B, n, A)), np.zeros((B, A))
        self.P = None   # the last solve's P [B, n, n, A], full and symmetric (not a record of the handle: for the tests of the theory)

    def _sel(self, mask):
        return np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)

    def set_model(self, a, q, r, mask=None):
        m = self._sel(mask)
        self.a[m], self.q[m], self.r[m] = np.asarray(a, dtype=np.float64)[m], np.asarray(q, dtype=np.float64)[m], np.asarray(r, dtype=np.float64)[m]
        for rec in (self.K, self.c, self.conv, self.solved, self.xhat, self.command):
            rec[m] = 0.0

    def _gain(self, P, r):
        """pc [n], K [n] from the upper triangle P[i][k], i <= k (each entry a [B', A] array)."""
        S, n = self.S, self.n
        at = lambda i, k: P[i][k] if i <= k else P[k][i]   # noqa: E731
        pc = []
        for i in range(n):
            acc = at(i, 0)
            for s in range(1, S):
                acc = acc + at(i, 2 * s)
            pc.append(acc)
        sv = pc[0]
        for s in range(1, S):
            sv = sv + pc[2 * s]
        sv = sv + r
        return pc, [pc[i] / sv for i in range(n)]

    def solve(self, delay, iterations, mask=None):
        """-> convergence [B, A] (rows of envs the mask leaves out: as they stood)."""
        S, n = self.S, self.n
        m = self._sel(mask)
        a1 = [self.a[m, s, 0] for s in range(S)]
        a2 = [self.a[m, s, 1] for s in range(S)]
        q = [self.q[m, s] for s in range(S)]
        r = self.r[m]
        zero = np.zeros_like(r)
        P = [[(q[i // 2].copy() if (i == k and i % 2 == 0) else zero.copy()) if i <= k else None for k in range(n)] for i in range(n)]

        def trace(P):
            t = P[0][0]
            for i in range(1, n):
                t = t + P[i][i]
            return t

        with np.errstate(all="ignore"):
            t_last = trace(P)
            t_prev = t_last
            for _ in range(int(iterations)):
                pc, K = self._gain(P, r)
                M = [[P[i][k] + (-(K[i] * pc[k])) if i <= k else None for k in range(n)] for i in range(n)]
                Pn = [[None] * n for _ in range(n)]
                for s in range(S):
                    for t in range(s, S):
                        m00, m01, m11 = M[2 * s][2 * t], M[2 * s][2 * t + 1], M[2 * s + 1][2 * t + 1]
                        m10 = M[2 * s][2 * s + 1] if s == t else M[2 * s + 1][2 * t]
                        n00 = (a1[s] * m00) + (a2[s] * m10)
                        n01 = (a1[s] * m01) + (a2[s] * m11)
                        p00 = (n00 * a1[t]) + (n01 * a2[t])
                        Pn[2 * s][2 * t] = p00 + q[s] if s == t else p00
                        Pn[2 * s][2 * t + 1] = n00
                        if s < t:
                            Pn[2 * s + 1][2 * t] = (m00 * a1[t]) + (m01 * a2[t])
                        Pn[2 * s + 1][2 * t + 1] = m00
                P = Pn
                t_prev = t_last
                t_last = trace(P)
            pc, K = self._gain(P, r)
            c = [np.ones_like(r) if i % 2 == 0 else zero.copy() for i in range(n)]
            for _ in range(int(delay)):
                for s in range(S):
                    c0 = c[2 * s]
                    c[2 * s] = (c0 * a1[s]) + c[2 * s + 1]
                    c[2 * s + 1] = c0 * a2[s]
            conv = np.abs(t_last + (-t_prev)) / t_last
            usable = r > 0.0
            for s in range(S):
                usable = usable & (np.abs(a2[s]) < 1.0) & (a1[s] + a2[s] < 1.0) & (a2[s] + (-a1[s]) < 1.0)
            conv = np.where(usable, conv, np.nan)
        self.K[m] = np.stack(K, axis=1)
        self.c[m] = np.stack(c, axis=1)
        self.conv[m] = conv
        self.solved[m] = 1.0
        full = np.stack([np.stack([P[min(i, k)][max(i, k)] for k in range(n)], axis=1) for i in range(n)], axis=1)   # [B', n, n, A]
        if self.P is None:
            self.P = np.zeros((self.B, n, n, self.A))
        self.P[m] = full
        return self.conv.copy()

    def update(self, y, mask=None):
        """-> out [B, A]: the command of every env as it stands after the call."""
        S, n = self.S, self.n
        y = np.asarray(y, dtype=np.float64)
        m = self._sel(mask) & np.isfinite(y).all(axis=1)
        x = [self.xhat[m, i] for i in range(n)]
        cx = x[0]
        for s in range(1, S):
            cx = cx + x[2 * s]
        e = y[m] + (-cx)
        xp = [x[i] + (self.K[m, i] * e) for i in range(n)]
        u = self.c[m, 0] * xp[0]
        for i in range(1, n):
            u = u + (self.c[m, i] * xp[i])
        new = np.empty_like(self.xhat[m])
        for s in range(S):
            new[:, 2 * s] = (self.a[m, s, 0] * xp[2 * s]) + (self.a[m, s, 1] * xp[2 * s + 1])
            new[:, 2 * s + 1] = xp[2 * s]
        self.xhat[m] = new
        self.command[m] = u
        return self.command.copy()

    def reset(self, mask=None):
        m = self._sel(mask)
        self.xhat[m] = 0.0
        self.command[m] = 0.0

    def blob(self):
        """The records in the handle's layout [B, 9 S + 4, A] float64."""
        B, A, S = self.B, self.A, self.S
        return np.concatenate([self.a.reshape(B, 2 * S, A), self.q, self.r[:, None], self.K, self.c, self.conv[:, None], self.solved[:, None], self.xhat,
                               self.command[:, None]], axis=1)


def prediction_variance(a, q, P, d):
    """C P_d C' of one (env, mode): P_1 = P (the Riccati solution, the one-step prediction covariance), P_{k+1} = A P_k A' + Q."""
    A_ = companion(a)
    n = A_.shape[0]
    Q = np.zeros((n, n))
    Q[np.arange(0, n, 2), np.arange(0, n, 2)] = q
    C = np.zeros(n)
    C[::2] = 1.0
    Pd = P.copy()
    for _ in range(d - 1):
        Pd = A_ @ Pd @ A_.T + Q
    return float(C @ Pd @ C)


def random_stable_model(rng, B, S, A, radius=0.98):
    """Random stable models: per sub-model a complex-conjugate pole pair or two real poles inside ``radius``; q and r in [1e-3, 1]."""
    rad1, rad2 = rng.uniform(0.1, radius, (B, S, A)), rng.uniform(0.1, radius, (B, S, A))
    theta = rng.uniform(0.0, np.pi, (B, S, A))
    pair = rng.uniform(size=(B, S, A)) < 0.5
    a1 = np.where(pair, 2.0 * rad1 * np.cos(theta), rad1 + rad2 * np.sign(np.cos(theta)))
    a2 = np.where(pair, -rad1 * rad1, -rad1 * rad2 * np.sign(np.cos(theta)))
    a = np.stack([a1, a2], axis=2)   # [B, S, 2, A]
    return np.ascontiguousarray(a), rng.uniform(1e-3, 1.0, (B, S, A)), rng.uniform(1e-3, 1.0, (B, A))
