"""Host restatement of the SPGD controller (aog_spgd_*, aog_reset_spgd / aog_step_spgd), written from include/aogym.h as the specification.
numpy only; nothing here touches the package's device path.

Two-sided SPGD with Bernoulli perturbations, per env: state u [A] float64, iteration k, half h, J_plus.

  delta_k: actuator i takes bit i & 31 of word (i >> 5) & 3 of Philox4x32-10 with counter (global env id, k, i >> 7, TAG), key = (seed low
  word, seed high word); a set bit is +1, a clear one -1.
  query, h = 0:  J_plus = J;  emit u - amplitude delta_k;  h = 1
  query, h = 1:  u = clip(u + (gain (J_plus - J)) delta_k);  k = k + 1;  h = 0;  emit u + amplitude delta_k (of the new k)
  reset:         u = 0 (or a given start);  h = 0;  k kept;  emit u + amplitude delta_k

J is a float32 widened to float64.  numpy's float64 array arithmetic rounds every product and sum once and fuses nothing, which is what the
library promises, so a replay from recorded metrics reproduces the device bit for bit.
"""
import numpy as np

TAG = 0x53504744
_M32 = (1 << 32) - 1


def philox4x32_10(counter, key):
    """Philox4x32-10 on Python integers: four counter words, two key words -> four output words."""
    c = [int(x) & _M32 for x in counter]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _M32, (p0 >> 32) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return c


def delta_bits(seed, env_id, k, act_dim):
    """The A perturbation bits of (global env id, iteration k) as a bool array: True = +1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    bits = np.zeros((act_dim,), dtype=bool)
    for call in range((act_dim + 127) // 128):
        words = philox4x32_10((env_id, k, call, TAG), (seed & _M32, seed >> 32))
        for i in range(128 * call, min(act_dim, 128 * call + 128)):
            bits[i] = (words[(i >> 5) & 3] >> (i & 31)) & 1
    return bits


def delta(seed, env_id, k, act_dim):
    """delta_k in {-1.0, +1.0}^A."""
    return np.where(delta_bits(seed, env_id, k, act_dim), 1.0, -1.0)


class SPGD:
    """The controller of ``num_envs`` envs with global ids ``env_id_base + row``.  ``gain`` / ``amplitude``: float64 [B]."""

    def __init__(self, num_envs, act_dim, gain, amplitude, seed, env_id_base=0, clip=0.0):
        self.B, self.A = int(num_envs), int(act_dim)
        self.gain = np.broadcast_to(np.asarray(gain, dtype=np.float64), (self.B,)).copy()
        self.amplitude = np.broadcast_to(np.asarray(amplitude, dtype=np.float64), (self.B,)).copy()
        self.seed, self.base, self.clip = int(seed), int(env_id_base), float(clip)
        self.u = np.zeros((self.B, self.A))
        self.k = np.zeros((self.B,), dtype=np.int64)
        self.h = np.zeros((self.B,), dtype=np.int64)
        self.J_plus = np.zeros((self.B,))

    def _delta(self, b):
        return delta(self.seed, self.base + b, int(self.k[b]), self.A)

    def reset(self, mask=None, start=None):
        """-> emitted commands float32 [B, A] (rows of unselected envs zero)."""
        out = np.zeros((self.B, self.A), dtype=np.float32)
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            self.u[b] = 0.0 if start is None else np.asarray(start, dtype=np.float64)[b]
            self.h[b] = 0
            out[b] = (self.u[b] + self.amplitude[b] * self._delta(b)).astype(np.float32)
        return out

    def update(self, metric, mask=None):
        """One query on ``metric`` (float32 [B]) -> emitted commands float32 [B, A]."""
        metric = np.asarray(metric)
        assert metric.dtype == np.float32 and metric.shape == (self.B,)
        out = np.zeros((self.B, self.A), dtype=np.float32)
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            J = np.float64(metric[b])
            if self.h[b] == 0:
                self.J_plus[b] = J
                out[b] = (self.u[b] - self.amplitude[b] * self._delta(b)).astype(np.float32)
                self.h[b] = 1
            else:
                step = self.gain[b] * (self.J_plus[b] - J)
                u = self.u[b] + step * self._delta(b)
                if self.clip > 0:
                    u = np.where(u > self.clip, self.clip, np.where(u < -self.clip, -self.clip, u))
                self.u[b] = u
                self.k[b] += 1
                self.h[b] = 0
                out[b] = (self.u[b] + self.amplitude[b] * self._delta(b)).astype(np.float32)
        return out
