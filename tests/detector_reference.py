"""Host restatement of the photodetector model of the observations (aog_set_detector), written from include/aogym.h and csrc/k_detector.h /
k_poisson.h as the specification.  numpy only; nothing here touches the package's device path.

Per (global env g, pixel j, frame f) the kernels make ONE Philox4x32-10 call, key = the handle's 64-bit rng_seed,
    counter = {j | 6 << 24,  g,  f & 0xFFFFFFFF,  (f >> 32) ^ 0xDE7EC7}
and, with c = the float32 clean power widened to float64, F photons, b background, sigma read noise:
    lam = F c + b
    lam < 12:  n = number of partial sums of the Poisson pmf that stay below u = (float32(word0 >> 8) + 0.5f) 2^-24 (1 - 4e-6f)   [float32]
    else:      n = max(0, rint(lam + float32(g sqrtf(lam) + (g g - 1) / 6))),  g = sqrt(-2 ln u1) cos(2 pi u2) in float32 from words 0, 1
    y = (n + sigma gr - b) / F,  gr the same Box-Muller form from words 2, 3;  obs_raw = float32(y), obs = float16(y)
The device walks the pmf in float32 and takes log / cos from the hardware, so a host value can differ where the uniform falls within a
hair of a step of the CDF or the rounded-normal argument within a hair of a half-integer: ``undecidable`` flags exactly those.
"""
import numpy as np

from actor_reference import philox4x32_10

TAG, FRAME_XOR = 6, 0xDE7EC7
SWITCH = 12.0
CDF_REL, HALF_ABS = 1e-5, 1e-6     # the undecidable rules: |u - CDF_k| <= CDF_REL CDF_k;  | |frac(arg)| - 1/2 | <= HALF_ABS
K_TERMS = 49                       # the device walks at most 48 terms past p_0


def detector_words(n_pix, env_ids, seed, frame, tag=TAG, frame_xor=FRAME_XOR):
    """uint32 [len(env_ids), n_pix, 4]: the four Philox words of every (env, pixel) of ``frame``."""
    seed, frame = int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(n_pix, dtype=np.int64)[None, :] | (int(tag) << 24)
    g = np.asarray(env_ids, dtype=np.int64)[:, None] & 0xFFFFFFFF
    w = philox4x32_10([j, g, frame & 0xFFFFFFFF, (frame >> 32) ^ frame_xor], [seed & 0xFFFFFFFF, seed >> 32])
    return np.stack(w, axis=-1)


def _u24(word, half):
    f = (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    if half:
        f = f + np.float32(0.5)
    return f * np.float32(2.0 ** -24)


def small_uniform(word):
    """The inversion's uniform, float32 arithmetic as the device's: ((word >> 8) + 0.5) 2^-24 (1 - 4e-6)."""
    return _u24(word, True) * (np.float32(1.0) - np.float32(4e-6))


def poisson_small(lam, word):
    """(n, undecidable) for lam < 12 by inversion against the float64 Poisson CDF."""
    lam = np.asarray(lam, dtype=np.float64)
    u = small_uniform(word).astype(np.float64)
    pk = np.exp(-lam)
    cdf = pk.copy()
    n = np.zeros(lam.shape, dtype=np.float64)
    und = np.zeros(lam.shape, dtype=bool)
    for k in range(1, K_TERMS + 1):
        n += u > cdf
        und |= np.abs(u - cdf) <= CDF_REL * cdf
        pk = pk * lam / k
        cdf = cdf + pk
    return n, und


def normal24(word_r, word_a, dtype=np.float32):
    """The cosine branch of the Box-Muller pair (radius word, angle word) from float32 uniforms, evaluated in ``dtype``.  The angle is a
    24-bit fraction of a REVOLUTION and the kernel hands it to the hardware cosine as such (k_poisson.h: ``cosf(u2)`` in revolutions): no
    product 2 pi u2 is ever rounded to float32.  So the cosine is taken of the exact angle and rounded once to ``dtype``; forming
    float32(2 pi) u2 in float32 first put up to 1.5e-6 between the float32 and the float64 evaluation of one pair, three times what the
    device's own normal differs from the float64 one by, and that times sqrt(lam) in poisson_large's argument."""
    u1, u2 = _u24(word_r, True).astype(dtype), _u24(word_a, False).astype(np.float64)
    return np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(2.0 * np.pi * u2).astype(dtype)


def poisson_large(lam, word_r, word_a):
    """(n, undecidable) for lam >= 12: rounded normal with the Cornish-Fisher term, float32 where the device is."""
    lam = np.asarray(lam, dtype=np.float64)
    g = normal24(word_r, word_a, np.float32)
    t = g * np.sqrt(lam.astype(np.float32)) + (g * g - np.float32(1.0)) * np.float32(1.0 / 6.0)
    arg = lam + t.astype(np.float64)
    frac = np.abs(arg - np.floor(arg) - 0.5)
    return np.maximum(0.0, np.rint(arg)), frac <= HALF_ABS


def expected_counts(clean, photons, background):
    """lam [B, n] = F c + b in float64 without fused multiply-add; clean = the noise-free handle's obs_raw (float32)."""
    c = np.asarray(clean, dtype=np.float32).astype(np.float64)
    return np.asarray(photons, dtype=np.float64)[:, None] * c + np.asarray(background, dtype=np.float64)[:, None]


def counts(lam, words):
    """(n, undecidable) [B, n] of the frame's words [B, n, 4]."""
    small = lam < SWITCH
    ns, us = poisson_small(np.where(small, lam, 0.0), words[..., 0])
    nl, ul = poisson_large(np.where(small, SWITCH, lam), words[..., 0], words[..., 1])
    return np.where(small, ns, nl), np.where(small, us, ul)


def read_normal(words, dtype=np.float64):
    return normal24(words[..., 2], words[..., 3], dtype)


def frame(clean, photons, read_noise, background, env_ids, seed, frame_index, **keying):
    """The detector's frame in float64: dict(y, n, lam, g, undecidable), each [B, n_pix]."""
    clean = np.asarray(clean)
    w = detector_words(clean.shape[1], env_ids, seed, frame_index, **keying)
    lam = expected_counts(clean, photons, background)
    n, und = counts(lam, w)
    g = read_normal(w)
    F, s, b = (np.asarray(a, dtype=np.float64)[:, None] for a in (photons, read_noise, background))
    return dict(y=(n + s * g - b) / F, n=n, lam=lam, g=g, undecidable=und)


def obs_of(y):
    """(obs_raw float32, obs float16) of float64 values, each rounded once from float64."""
    y = np.asarray(y, dtype=np.float64)
    return y.astype(np.float32), y.astype(np.float16)
