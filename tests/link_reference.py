"""A plain numpy / ``math`` restatement of the link telemetry's definitions (``include/aogym.h``, aog_link_statistics), on one env's
chronological window: Python loops for the runs, ``math.fsum`` for the sums, ``math.erfc`` for the bit-error rate.  Beside it the
segment summary and its merge as ``csrc/k_link.h`` states them, so that the combination rule itself has a test without a device."""
import math

import numpy as np


def db(values):
    """dB -> linear factors, as the Python layer converts them."""
    return np.power(10.0, np.asarray(values, dtype=np.float64) / 10.0)


def window(ring, count):
    """The last min(count, T) samples of a ring (sample c at c mod T), oldest first."""
    ring = np.asarray(ring, dtype=np.float32)
    T = ring.size
    n = max(0, min(int(count), T))
    return np.array([ring[c % T] for c in range(int(count) - n, int(count))], dtype=np.float32)


def runs(in_fade):
    """(samples in fade, maximal runs of consecutive in-fade samples, the longest run) of a sequence of booleans."""
    below = fades = longest = cur = 0
    for f in in_fade:
        if f:
            below += 1
            cur += 1
            if cur == 1:
                fades += 1
            longest = max(longest, cur)
        else:
            cur = 0
    return below, fades, longest


def statistics(win, reference, factors=(), hist_factors=(), q=()):
    """Every output of aog_link_statistics for one window.  ``reference``: "mean" or the absolute level; the factors are linear."""
    p = [float(v) for v in np.asarray(win, dtype=np.float32)]   # (float32 -> float64 is exact)
    n, K, E, Q = len(p), len(factors), len(hist_factors), len(q)
    nan = float("nan")
    if n == 0:
        return dict(samples=0, mean=nan, mean_square=nan, scintillation_index=nan, minimum=nan, maximum=nan, reference=nan, below=[0] * K,
                    fades=[0] * K, longest=[0] * K, hist=[0] * (E + 1), ber=[nan] * Q, edges=[], hist_edges=[])
    mean = math.fsum(p) / n
    mean_square = math.fsum(v * v for v in p) / n   # (a float32 squared is exact in float64)
    P = mean if isinstance(reference, str) else float(reference)
    edges = [P * float(f) for f in factors]
    hist_edges = [P * float(g) for g in hist_factors]
    below, fades, longest = (list(c) for c in zip(*[runs(v < e for v in p) for e in edges])) if K else ([], [], [])
    hist = [0] * (E + 1)
    for v in p:
        j = 0
        while j < E and v >= hist_edges[j]:
            j += 1
        hist[j] += 1
    ber = [math.fsum(0.5 * math.erfc(float(qm) * v / (P * math.sqrt(2.0))) for v in p) / n for qm in q]
    return dict(samples=n, mean=mean, mean_square=mean_square, scintillation_index=mean_square / (mean * mean) - 1.0, minimum=min(p), maximum=max(p),
                reference=P, below=below, fades=fades, longest=longest, hist=hist, ber=ber, edges=edges, hist_edges=hist_edges)


def edge_margin(win, stats):
    """The smallest relative distance |p - e| / e between any sample and any threshold or histogram edge (inf without samples or edges)."""
    p = np.asarray(win, dtype=np.float64)
    e = np.asarray(list(stats["edges"]) + list(stats["hist_edges"]), dtype=np.float64)
    if p.size == 0 or e.size == 0:
        return float("inf")
    return float(np.min(np.abs(p[:, None] - e[None, :]) / np.abs(e[None, :])))


# ---- the second formulation: no running state, only positions ---------------------------------------------------------------------------
def runs_brute(in_fade):
    """The same three numbers from the text of the sequence: the pieces between the samples out of fade."""
    text = "".join("1" if f else "0" for f in in_fade)
    pieces = [piece for piece in text.split("0") if piece]
    return text.count("1"), len(pieces), max((len(piece) for piece in pieces), default=0)


def hist_brute(win, hist_edges):
    p = np.asarray(win, dtype=np.float64)
    e = np.asarray(hist_edges, dtype=np.float64)
    return np.bincount(np.searchsorted(e, p, side="right"), minlength=e.size + 1).tolist()


# ---- the kernel's combination rule ---------------------------------------------------------------------------------------------------
def segment(in_fade):
    """A stretch of the window as (length, below, runs, prefix run, suffix run, longest run)."""
    f = [bool(v) for v in in_fade]
    below, fades, longest = runs(f)
    prefix = next((i for i, v in enumerate(f) if not v), len(f))
    suffix = next((i for i, v in enumerate(reversed(f)) if not v), len(f))
    return (len(f), below, fades, prefix, suffix, longest)


def merge(left, right):
    """``left`` then ``right``: two runs that touch fuse into one; the empty stretch is the identity."""
    ll, lb, lr, lp, ls, lg = left
    rl, rb, rr, rp, rs, rg = right
    return (ll + rl, lb + rb, lr + rr - (1 if ls > 0 and rp > 0 else 0), ll + rp if lb == ll else lp, rl + ls if rb == rl else rs, max(lg, rg, ls + rp))


def merged_runs(in_fade, chunk):
    """(below, fades, longest) through chunks of ``chunk`` samples merged by a tree in the kernel's order (lane l takes lane l + 2^s)."""
    f = list(in_fade)
    lanes = [segment(f[i * chunk:(i + 1) * chunk]) for i in range(64)]
    assert 64 * chunk >= len(f)
    off = 1
    while off < 64:
        for lane in range(0, 64, 2 * off):
            lanes[lane] = merge(lanes[lane], lanes[lane + off])
        off *= 2
    return lanes[0][1], lanes[0][2], lanes[0][5]


class RingReference:
    """push / reset of aog_link on the host: float32 rings, a non-finite sample skipped and counted."""

    def __init__(self, B, T):
        self.ring = np.zeros((B, T), dtype=np.float32)
        self.count = np.zeros(B, dtype=np.int64)
        self.skipped = np.zeros(B, dtype=np.int64)

    def push(self, power, mask=None):
        for b, v in enumerate(np.asarray(power, dtype=np.float32)):
            if mask is not None and not mask[b]:
                continue
            if not np.isfinite(v):
                self.skipped[b] += 1
                continue
            self.ring[b, self.count[b] % self.ring.shape[1]] = v
            self.count[b] += 1

    def reset(self, mask=None):
        for b in range(self.ring.shape[0]):
            if mask is None or mask[b]:
                self.ring[b] = 0
                self.count[b] = self.skipped[b] = 0

    def window(self, b):
        return window(self.ring[b], self.count[b])
