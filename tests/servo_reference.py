"""Host restatement of the mirror servo (a helper: nothing here is collected), written from the text of ``include/aogym_servo.h``: numpy
float64, one rounded operation per line of the header, no fused multiply-add (numpy has none).  The GPU tests hold ``aog_servo_apply`` to
it bit for bit."""
import numpy as np


class Servo:
    """``latency``, ``response``, ``stroke`` [B] float64 (``stroke`` +inf: none); ``stuck`` [B, A] bool, ``stuck_value`` [B, A] float32.
    State: ``y`` [B, A] float64, ``ring`` [B, R, A] float32 with R = max_latency + 2, ``n`` the handle's call counter."""

    def __init__(self, B, A, max_latency, latency=0.0, response=1.0, stroke=np.inf, stuck=None, stuck_value=None):
        self.B, self.A, self.R = int(B), int(A), int(max_latency) + 2
        self.latency = np.broadcast_to(np.asarray(latency, dtype=np.float64), (B,)).copy()
        self.response = np.broadcast_to(np.asarray(response, dtype=np.float64), (B,)).copy()
        self.stroke = np.broadcast_to(np.asarray(stroke, dtype=np.float64), (B,)).copy()
        assert np.all(self.latency >= 0) and np.all(self.latency <= max_latency) and np.all(self.response > 0) and np.all(self.response <= 1)
        assert np.all(self.stroke > 0)
        self.stuck = np.zeros((B, A), dtype=bool) if stuck is None else np.broadcast_to(np.asarray(stuck, dtype=bool), (B, A)).copy()
        self.stuck_value = (np.zeros((B, A), dtype=np.float32) if stuck_value is None
                            else np.broadcast_to(np.asarray(stuck_value, dtype=np.float32), (B, A)).copy())
        self.y = np.zeros((B, A), dtype=np.float64)
        self.ring = np.zeros((B, self.R, A), dtype=np.float32)
        self.n = 0

    def reset(self, mask=None):
        sel = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.y[sel] = 0.0
        self.ring[sel] = 0.0

    def apply(self, action, mask=None, out=None):
        """One call: returns action_out [B, A] float32 (``out``, or zeros, with the rows of the envs the mask leaves out untouched)."""
        action = np.asarray(action, dtype=np.float32)
        assert action.shape == (self.B, self.A)
        sel = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        out = np.zeros((self.B, self.A), dtype=np.float32) if out is None else out
        n, R = self.n, self.R
        for b in np.flatnonzero(sel):
            self.ring[b, n % R] = action[b]                               # 1.
            d = int(np.floor(self.latency[b]))                            # 2.
            f = self.latency[b] - d
            c = self.ring[b, (n - d) % R].astype(np.float64)
            if f != 0.0:
                older = self.ring[b, (n - d - 1) % R].astype(np.float64)
                w = 1.0 - f
                p0 = w * c
                p1 = f * older
                c = p0 + p1
            s = self.stroke[b]                                            # 3.
            if s < np.inf:
                c = np.where(c < -s, -s, c)
                c = np.where(c > s, s, c)
            r = self.response[b]                                          # 4.
            if r == 1.0:
                y = c.copy()
            else:
                diff = c - self.y[b]
                move = r * diff
                y = self.y[b] + move
            self.y[b] = y
            with np.errstate(over="ignore"):
                out[b] = np.where(self.stuck[b], self.stuck_value[b], y.astype(np.float32))   # 5. (numpy's cast rounds to nearest even)
        self.n += 1
        return out

    def blob(self):
        """The checkpoint blob: y, the counter, the ring."""
        return np.concatenate([self.y.ravel().view(np.uint8), np.array([self.n], dtype=np.uint64).view(np.uint8), self.ring.ravel().view(np.uint8)])
