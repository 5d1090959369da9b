"""Host restatement of the Shack-Hartmann camera's photon-noise stream, written from csrc/k_poisson.h (sh_noise_words and the sampler) and
sh_noisy_value in csrc/k_shack.h as the specification.  numpy only; nothing here touches the package's device path.  The sampler itself
(poisson_small, poisson_large and the undecidable rules CDF_REL / HALF_ABS) is detector_reference's, Philox is actor_reference's.

Pixel (global env ge, row y, column x) of an N x N camera takes word ``r & 3`` of the Philox4x32-10 call with
    counter = {lo32(line),  hi32(line) ^ (group << 20) ^ (second ? 0x80000000 : 0),  call,  0x50155},   key = the handle's 64-bit rng_seed
    row-keyed form (sep_rl = 0):     line = (ge N + y) 64 + (x % LW),  r = x / LW,   LW = 60 for pupils of 60 R pixels, else 64
    separable-route form (sep_rl):   line = (ge N + x) 64 + (y % RL),  r = y / RL,   RL = sep_rl
    group = r >> 2
lam < 12 inverts the Poisson CDF on that word; brighter pixels take it as the Box-Muller radius and the same word of a SECOND call (flag
bit set) as the angle.  ``call`` is the handle's sh_calls: 0 at creation, incremented by ONE before every draw (csrc/shack.hip: aog_sh_image
without an image on the fused routes, aog_sh_update(null) otherwise), so the first draw of a handle uses call 1.

``Key`` spells the layout out as data; ``WRONG_KEYS`` are the mistakes the tests must be able to tell from it.
"""
import collections

import numpy as np

import detector_reference as dr
from actor_reference import philox4x32_10

TAG = 0x50155
FIRST_CALL, CALL_STEP = 1, 1     # csrc/shack.hip: sh_calls = 0 in the fresh handle, `e->sh_calls += 1` ahead of each draw

# lw: None = the rule of spectrum_lane_width, or a forced width; the other fields exist only to state WRONG keys
Key = collections.namedtuple("Key", "lw group_zero drop_second swap_axes env_add call_add")
KEY = Key(lw=None, group_zero=False, drop_second=False, swap_axes=False, env_add=0, call_add=0)


def lane_width(N):
    """spectrum_lane_width (csrc/k_common.h): 60 for pupils of 60 R pixels that are no multiple of 64, else 64."""
    return 60 if (N % 64 != 0 and N % 60 == 0) else 64


def wrong_keys(N, sep_rl=0, env_base=0):
    """name -> Key for the mistakes of the issue.  The lane width enters the row-keyed form only; ``local_env`` needs env_base > 0."""
    out = collections.OrderedDict()
    if not sep_rl:
        out["lane_width_64_60_swapped"] = KEY._replace(lw=124 - lane_width(N))
    out["group_forced_to_0"] = KEY._replace(group_zero=True)
    out["second_flag_dropped"] = KEY._replace(drop_second=True)
    out["axes_exchanged"] = KEY._replace(swap_axes=True)
    if env_base:
        out["local_env_id"] = KEY._replace(env_add=-int(env_base))
    out["call_plus_1"] = KEY._replace(call_add=1)
    return out


def pixel_lines(N, env_ids, sep_rl=0, key=KEY):
    """(line uint64 [E, N, N], r int64 [1, N, N]) of every pixel: the Philox line it draws from and its index along that line's lane."""
    y, x = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(N, dtype=np.int64), indexing="ij")
    if key.swap_axes:
        y, x = x, y
    ge = (np.asarray(env_ids, dtype=np.int64) + key.env_add).astype(np.uint64)[:, None, None]
    if sep_rl:
        along, lane, r = x, y % sep_rl, y // sep_rl
    else:
        lw = key.lw if key.lw is not None else lane_width(N)
        along, lane, r = y, x % lw, x // lw
    line = (ge * np.uint64(N) + along.astype(np.uint64)[None]) * np.uint64(64) + lane.astype(np.uint64)[None]
    return line, r[None]


def sh_words(N, env_ids, seed, call, sep_rl=0, second=False, key=KEY):
    """uint32 [E, N, N]: the Philox word every pixel takes (``second``: of the bright pixels' second call)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    line, r = pixel_lines(N, env_ids, sep_rl, key)
    group = np.zeros_like(r) if key.group_zero else r >> 2
    c0 = line & np.uint64(0xFFFFFFFF)                                         # the 64-bit line: low word into counter 0,
    c1 = (line >> np.uint64(32)) ^ (group.astype(np.uint64) << np.uint64(20))  # high word XORed into counter 1 beside group and flag
    if second and not key.drop_second:
        c1 = c1 ^ np.uint64(0x80000000)
    w = philox4x32_10([c0, c1 & np.uint64(0xFFFFFFFF), (int(call) + key.call_add) & 0xFFFFFFFF, TAG], [seed & 0xFFFFFFFF, seed >> 32])
    w = np.stack(w, axis=-1)                                                   # [E, N, N, 4]
    sel = np.broadcast_to((r & 3)[..., None], w.shape[:3] + (1,))
    return np.take_along_axis(w, sel, axis=-1)[..., 0]


def noisy_image(lam, env_ids, seed, call, sep_rl=0, key=KEY):
    """(counts, undecidable), each [E, N, N]: sh_noisy_value of every pixel of the expectations ``lam`` [E, N, N] float64."""
    lam = np.asarray(lam, dtype=np.float64)
    E, N, _ = lam.shape
    assert lam.shape == (len(env_ids), N, N)
    w1 = sh_words(N, env_ids, seed, call, sep_rl, False, key)
    w2 = sh_words(N, env_ids, seed, call, sep_rl, True, key)
    small = lam < dr.SWITCH
    ns, us = dr.poisson_small(np.where(small, lam, 0.0), w1)
    nl, ul = dr.poisson_large(np.where(small, dr.SWITCH, lam), w1, w2)
    return np.where(small, ns, nl), np.where(small, us, ul)


EDGE_ROWS = ((8, 16, 0.0), (16, 24, float(np.nextafter(12.0, 0.0))), (24, 32, 12.0))   # (first row, end row, lam) of the overwritten row blocks


def lam_field(n_env, n, seed=2024):
    """The test field: 10 ** uniform(-3, 4) per pixel, whole row blocks overwritten with 0, the last double below the switch and the switch."""
    lam = 10.0 ** np.random.RandomState(seed).uniform(-3.0, 4.0, (n_env, n, n))
    for lo, hi, v in EDGE_ROWS:
        lam[:, lo:hi, :] = v
    return lam
