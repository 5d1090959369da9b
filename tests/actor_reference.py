"""Host restatement of the policy query (aog_actor_act / aog_actor_act_noise and the fused step tail), written from include/aogym.h and
csrc/k_actor.h as the specification.  numpy only; nothing here touches the package's device path.

The kernels draw every random word from counter-based Philox4x32-10, so the host can regenerate each word the device used:

  unit m of stream tag L (1..3 = dropout mask of hidden layer L, 4 = eps of the output layer, 5 = the Ornstein-Uhlenbeck normals),
  global env g = env_id_base + row, 64-bit seed and call_index:
      counter = {(m & ~3) | L << 24,  g,  call_index & 0xFFFFFFFF,  (call_index >> 32) ^ 0xAC70},  key = {seed & 0xFFFFFFFF, seed >> 32};
      unit m takes word m & 3 of the four.
  hidden layers: u = float32(word >> 8) * 2^-24 in [0, 1); kept iff u >= float32(dropout_p), then multiplied by keep_scale = 1 / (1 - p) in float32.
  tags 4 and 5:  words (2h, 2h + 1) of a group give units m0 + 2h (cosine) and m0 + 2h + 1 (sine) of one Box-Muller pair with
      u = (float32(word) + 0.5f) * 2^-32 in float32 (u1 in (0, 1], it may round to exactly 1), normal = sqrt(-2 ln u1) {cos, sin}(2 pi u2).

``Keying`` spells that layout out as data; the wrong variants in ``WRONG_KEYINGS`` are what the tests must be able to tell from it.  ``CASES``
is the one table both test files iterate.  The ``check_*`` functions are the comparisons the GPU tests apply to device output; the CPU tests
feed them wrongly keyed references to show that they reject them.
"""
import collections
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) vectorised over numpy arrays: ``counter`` four and ``key`` two broadcastable arrays of 32-bit
    values; returns the four output words as uint32 arrays.  uint64 arithmetic masked to 32 bits."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    k0, k1 = [np.asarray(x, dtype=np.uint64) & M32 for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0 = PHILOX_M0 * c[0]   # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return [x.astype(np.uint32) for x in c]


# The keying of the query as data.  tags: stream tag of hidden layers 1..3, of eps and of the OU normals; the *_add / *_xor fields and
# group_mask / swap_cos_sin exist only to state WRONG keyings.
Keying = collections.namedtuple("Keying", "tags call_add seed_xor env_add group_mask swap_cos_sin")
KEYING = Keying(tags=(1, 2, 3, 4, 5), call_add=0, seed_xor=0, env_add=0, group_mask=~3, swap_cos_sin=False)
# name -> (keying, what it must move: "mean" (dropout masks), "eps", or both)
WRONG_KEYINGS = collections.OrderedDict([
    ("tags_2_3_swapped", (KEYING._replace(tags=(1, 3, 2, 4, 5)), ("mean",))),
    ("call_index_plus_1", (KEYING._replace(call_add=1), ("mean", "eps"))),
    ("call_index_plus_2^32", (KEYING._replace(call_add=1 << 32), ("mean", "eps"))),
    ("seed_xor_2^32", (KEYING._replace(seed_xor=1 << 32), ("mean", "eps"))),
    ("env_id_base_plus_1", (KEYING._replace(env_add=1), ("mean", "eps"))),
    ("unit_group_of_16", (KEYING._replace(group_mask=~15), ("mean",))),
    ("cos_sin_swapped", (KEYING._replace(swap_cos_sin=True), ("eps",))),
])


def stream_words(tag, n_units, env_ids, seed, call_index, keying=KEYING):
    """uint32 [len(env_ids), n_units]: the Philox word of every (env, unit) under stream ``tag``."""
    seed = (int(seed) ^ keying.seed_xor) & 0xFFFFFFFFFFFFFFFF
    call = (int(call_index) + keying.call_add) & 0xFFFFFFFFFFFFFFFF
    m = np.arange(n_units, dtype=np.int64)
    c0 = ((m & keying.group_mask) | (int(tag) << 24))[None, :]
    g = (np.asarray(env_ids, dtype=np.int64) + keying.env_add)[:, None] & 0xFFFFFFFF
    words = philox4x32_10([c0, g, call & 0xFFFFFFFF, (call >> 32) ^ 0xAC70], [seed & 0xFFFFFFFF, seed >> 32])
    words = np.stack(words, axis=-1)                                  # [B, n_units, 4]
    return np.take_along_axis(words, np.broadcast_to((m & 3)[None, :, None], words.shape[:2] + (1,)), axis=-1)[..., 0]


def mask_uniform(words):
    """The hidden layers' uniform: float32(word >> 8) * 2^-24, in [0, 1)."""
    return (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(words, dropout_p):
    """True where the unit is kept: u >= float32(dropout_p)."""
    return mask_uniform(words) >= np.float32(dropout_p)


def keep_scale(dropout_p):
    """float32(1) / (float32(1) - float32(dropout_p)), in float32 arithmetic."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(dropout_p))


def normal_uniform(words):
    """Box-Muller's uniform: (float32(word) + 0.5f) * 2^-32 in float32 arithmetic, in (0, 1] (the largest words round to exactly 1)."""
    return (np.asarray(words, dtype=np.uint32).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def normals(words, swap_cos_sin=False, dtype=np.float64):
    """Standard normals [B, n] from words [B, n]: words (2h, 2h + 1) of a group of four are (u1, u2) of one pair, unit 2h takes the cosine
    and unit 2h + 1 the sine.  Evaluated in ``dtype`` from the float32 uniforms."""
    words = np.asarray(words, dtype=np.uint32)
    B, n = words.shape
    npad = (n + 3) // 4 * 4
    # (a unit's partner word lives in the same Philox call, also when the partner is past the layer's end: stream_normals pads and cuts)
    assert n == npad, "normals() needs whole groups of four words"
    u = normal_uniform(words).astype(dtype)
    u1, u2 = u[:, 0::2], u[:, 1::2]
    two_pi = dtype(2.0 * math.pi)
    rad = np.sqrt(dtype(-2.0) * np.log(u1))
    c, s = rad * np.cos(two_pi * u2), rad * np.sin(two_pi * u2)
    if swap_cos_sin:
        c, s = s, c
    out = np.empty((B, n), dtype=dtype)
    out[:, 0::2], out[:, 1::2] = c, s
    return out


def stream_normals(tag, n_units, env_ids, seed, call_index, keying=KEYING, dtype=np.float64):
    npad = (n_units + 3) // 4 * 4
    return normals(stream_words(tag, npad, env_ids, seed, call_index, keying), keying.swap_cos_sin, dtype)[:, :n_units]


def widen_obs(obs):
    """The observation as the kernel reads it: float16 bits widened, or float32; float64 array."""
    obs = np.asarray(obs)
    assert obs.dtype in (np.float16, np.float32), obs.dtype
    return obs.astype(np.float64)


def masked_mlp(weights, x, masks, scale, dtype=np.float64):
    """mean = W_o d3(relu(W_3 d2(relu(W_2 d1(relu(W_1 x + b_1)) + b_2)) + b_3)) + b_o with d_l(v) = v * masks[l] * scale, in ``dtype``."""
    w = [np.asarray(a, dtype=np.float32).astype(dtype) for a in weights]
    x = np.asarray(x).astype(dtype)
    for layer in range(3):
        x = np.maximum(x @ w[2 * layer].T + w[2 * layer + 1], dtype(0)) * masks[layer].astype(dtype) * dtype(scale)
    return x @ w[6].T + w[7]


Query = collections.namedtuple("Query", "mean eps action log_prob ou_state masks mean_f32_spread")


def reference_query(weights, obs, dropout_p, cov_var, seed, call_index, env_id_base=0, mode="sample", ou_state=None, mu=0.0, theta=0.0,
                    sigma=0.0, keying=KEYING):
    """The policy query in float64.  weights: (w1, b1, w2, b2, w3, b3, wo, bo) float32 in nn.Linear layout; obs [B, S] float16 or float32.
    Returns Query(mean [B, A], eps [B, A], action [B, A], log_prob [B], new OU state [B, A] or None, the three keep masks,
    the largest deviation of a float32 numpy evaluation of the same masked network from the float64 one).  With an OU state the action is
    float32(float64(g) + s') as the kernel forms it, g = float32(mean + sqrt(cov_var) eps) (mean mode: float32(mean))."""
    x = widen_obs(obs)
    B = x.shape[0]
    H, A = weights[0].shape[0], weights[6].shape[0]
    env_ids = int(env_id_base) + np.arange(B)
    masks = [keep_mask(stream_words(keying.tags[layer], H, env_ids, seed, call_index, keying), dropout_p) for layer in range(3)]
    scale = keep_scale(dropout_p)
    mean = masked_mlp(weights, x, masks, scale)
    spread = float(np.max(np.abs(masked_mlp(weights, x, masks, scale, np.float32).astype(np.float64) - mean))) if mean.size else 0.0
    eps = stream_normals(keying.tags[3], A, env_ids, seed, call_index, keying)
    cov = float(np.float32(cov_var))
    logp_const = 0.5 * A * math.log(2.0 * math.pi * cov)
    if mode == "mean":
        action, log_prob = mean.copy(), np.full(B, -logp_const)
    else:
        assert mode == "sample", mode
        action = mean + math.sqrt(cov) * eps
        log_prob = -0.5 * np.sum(eps * eps, axis=1) - logp_const
    new_state = None
    if ou_state is not None:
        n = stream_normals(keying.tags[4], A, env_ids, seed, call_index, keying)
        s = np.asarray(ou_state, dtype=np.float64)
        new_state = s + (theta * (mu - s) + sigma * n)
        action = (action.astype(np.float32).astype(np.float64) + new_state).astype(np.float32).astype(np.float64)
    return Query(mean, eps, action, log_prob, new_state, masks, spread)


# ---- the comparisons the GPU tests apply to device output --------------------------------------------------------------------------------------
MEAN_RTOL, MEAN_ATOL = 2e-5, 2e-6          # the project's tolerance of this kernel at p = 0 (test_device_actor_matches_torch_module)
F32_SPREAD_FACTOR = 8.0                    # allowance of the cases listed in F32_SPREAD_CASES: a multiple of a float32 evaluation's own spread
EPS_F32_BOX_MULLER = 1.5e-6                # float32 numpy Box-Muller against float64 on the same words (2 M words, |eps| up to 5)
EPS_TOL = 16 * EPS_F32_BOX_MULLER          # 2.4e-5: approximate instead of correctly rounded hardware transcendentals, radius up to 6.8
EPS_CEILING = 1e-4                         # a keying mistake is an O(1) error on a unit-variance number
LOGP_RTOL, LOGP_ATOL = 1e-4, 1e-3


def mean_bound(ref, f32_spread=None):
    """Elementwise allowance on the mean: MEAN_RTOL |ref| + MEAN_ATOL max(1, max |ref|); with ``f32_spread`` (a case of
    F32_SPREAD_CASES) F32_SPREAD_FACTOR times the float32 evaluation's spread instead."""
    ref = np.asarray(ref, dtype=np.float64)
    if f32_spread is not None:
        return np.full(ref.shape, F32_SPREAD_FACTOR * f32_spread)
    return MEAN_RTOL * np.abs(ref) + MEAN_ATOL * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)


def _note(log, what, **figures):
    """Append a check's figures to ``log`` (a list, or None) BEFORE the check asserts, so that a failing run still reports them."""
    if log is not None:
        log.append((what, figures))


def check_mean(mean_dev, ref, f32_spread=None, what="mean", log=None):
    """Every element of the device mean within mean_bound of the float64 reference.  Returns the largest fraction of the bound used."""
    dev = np.asarray(mean_dev, dtype=np.float64)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    frac = np.abs(dev - ref) / mean_bound(ref, f32_spread)
    worst = float(np.nanmax(frac)) if np.all(np.isfinite(dev)) else float("inf")
    _note(log, what, frac=worst, max_abs_ref=float(np.max(np.abs(ref))))
    assert worst <= 1.0, f"{what}: {int((~(frac <= 1)).sum())} of {frac.size} elements out of tolerance, worst {worst:.3g} x the bound"
    return worst


def device_std(cov_var):
    """sqrt(cov_var) as actor_args computes it (float32)."""
    return float(np.sqrt(np.float32(cov_var)))


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def eps_bound(action_dev, std, ou_state_dev=None):
    """EPS_TOL plus the rounding of recovering eps from the float32 action, ulp32(|action|) / std; never above EPS_CEILING.  With an OU
    state the kernel rounded twice (g = float32(mean + std eps), action = float32(g + s)): ulp32(|action|) + ulp32(|action - s|)."""
    ulp = _ulp32(action_dev)
    if ou_state_dev is not None:
        ulp = ulp + _ulp32(np.asarray(action_dev, dtype=np.float64) - ou_state_dev)
    return np.minimum(EPS_TOL + ulp / std, EPS_CEILING)


def device_eps(action_dev, mean_dev, cov_var, ou_state_dev=None):
    """eps recovered from device output: (action [- OU state] - mean) / sqrt(cov_var) in float64 on the device's outputs."""
    g = np.asarray(action_dev, dtype=np.float64)
    if ou_state_dev is not None:
        g = g - ou_state_dev
    return (g - np.asarray(mean_dev, dtype=np.float64)) / device_std(cov_var)


def check_eps(action_dev, mean_dev, cov_var, ref_eps, what="eps", log=None, ou_state_dev=None, recovery=True):
    """Every recovered eps within eps_bound of the reference (recovery=False: within EPS_TOL alone, for a query whose mean is exactly
    zero).  Returns (largest fraction of the bound used, largest deviation)."""
    eps = device_eps(action_dev, mean_dev, cov_var, ou_state_dev)
    assert eps.shape == ref_eps.shape, what
    err = np.abs(eps - ref_eps)
    frac = err / (eps_bound(action_dev, device_std(cov_var), ou_state_dev) if recovery else EPS_TOL)
    ok = bool(np.all(np.isfinite(eps)))
    worst, dev = (float(frac.max()), float(err.max())) if ok else (float("inf"), float("inf"))
    _note(log, what, frac=worst, deviation=dev, max_abs_eps=float(np.max(np.abs(ref_eps))))
    assert worst <= 1.0, f"{what}: {int((~(frac <= 1)).sum())} of {frac.size} elements out of tolerance, worst {worst:.3g} x the bound (deviation {dev:.3g})"
    return worst, dev


def eps_differs(action_dev, mean_dev, cov_var, other_eps):
    """True when the recovered eps is NOT within tolerance of ``other_eps`` (another call's stream) on most elements."""
    err = np.abs(device_eps(action_dev, mean_dev, cov_var) - other_eps)
    return float(np.mean(err > EPS_CEILING)) > 0.9


def check_log_prob(log_prob_dev, ref_log_prob, what="log_prob", log=None):
    dev = np.asarray(log_prob_dev, dtype=np.float64)
    assert dev.shape == ref_log_prob.shape, what
    frac = np.abs(dev - ref_log_prob) / (LOGP_ATOL + LOGP_RTOL * np.abs(ref_log_prob))
    worst = float(frac.max()) if np.all(np.isfinite(dev)) else float("inf")
    _note(log, what, frac=worst)
    assert worst <= 1.0, f"{what}: worst {worst:.3g} x the bound"
    return worst


def check_ou_state(state_dev, ref_state, sigma, what="OU state", log=None):
    """The new OU state against the float64 recursion: sigma x EPS_TOL (the state is float64: nothing to recover); sigma = 0: exactly equal.
    Returns the largest fraction of the bound used (0 for sigma = 0)."""
    dev = np.asarray(state_dev, dtype=np.float64)
    assert dev.shape == ref_state.shape, what
    if sigma == 0.0:
        np.testing.assert_array_equal(dev, ref_state, err_msg=what)
        return 0.0
    frac = np.abs(dev - ref_state) / (sigma * EPS_TOL)
    worst = float(frac.max()) if np.all(np.isfinite(dev)) else float("inf")
    _note(log, what, frac=worst)
    assert worst <= 1.0, f"{what}: worst {worst:.3g} x the bound"
    return worst


PREACT_MARGIN = 1e-3


def zero_pattern(weights_identity, obs, masks):
    """For the identity construction (layers 2, 3 = identity, out = the first A rows of the identity, no bias there): which means must be
    exactly zero (a unit dropped in any of the three layers, or a layer-1 pre-activation below -PREACT_MARGIN) and which must not be
    (kept three times and a pre-activation above PREACT_MARGIN).  Elements in neither set (|pre-activation| <= PREACT_MARGIN: a float32
    sum may land on either side of zero) are left to the comparison of the mean, which covers every element."""
    A = weights_identity[6].shape[0]
    pre = widen_obs(obs) @ weights_identity[0].astype(np.float64).T + weights_identity[1].astype(np.float64)
    pre = pre[:, :A]
    kept = masks[0][:, :A] & masks[1][:, :A] & masks[2][:, :A]
    return ~kept | (pre < -PREACT_MARGIN), kept & (pre > PREACT_MARGIN)


def check_zero_pattern(mean_dev, must_be_zero, must_be_nonzero, what="zero pattern"):
    dev = np.asarray(mean_dev)
    z = dev == 0
    assert not np.any(must_be_zero & ~z), f"{what}: {int((must_be_zero & ~z).sum())} dropped / negative units have a nonzero mean"
    assert not np.any(must_be_nonzero & z), f"{what}: {int((must_be_nonzero & z).sum())} kept positive units have a zero mean"


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name S H A B p env_id_base seed call_index wseed out_scale")


def _case(name, S, H, A, B, p=0.5, env_id_base=0, seed=5, call_index=0, wseed=0, out_scale=100.0):
    return Case(name, S, H, A, B, p, env_id_base, seed, call_index, wseed, out_scale)


# wseed / out_scale: the weights' seed and the factor on the output layer's reference initialisation (3e-3), chosen so that the REFERENCE alone
# meets the discriminating-power condition of test_actor_reference_cpu.py (never from device output).
CASES = [
    _case("reference_shape_ragged", 4, 150, 64, 1000),
    _case("o5", 25, 150, 20, 37),
    _case("one_tile_odd_one_env", 9, 37, 1, 1),
    _case("act_dim_6_p09", 4, 32, 6, 5, p=0.9, seed=7),   # seed 5 drops every unit of one env under two keyings alike
    _case("weight_chunks_h400", 9, 400, 100, 33),
    _case("state_256_over_hidden", 256, 150, 64, 20),
    _case("separable_obs_1024", 1024, 150, 64, 20),
    _case("hidden_496_beside_1024", 1024, 496, 16, 17),
    _case("hidden_848_widest", 4, 848, 16, 16),
    _case("keying_fields", 4, 150, 16, 70, env_id_base=12345, seed=0x1234567890ABCDEF, call_index=(1 << 32) + 7),
    _case("p0_regression", 4, 150, 64, 70, p=0.0),
]
# (S, H) that aog_actor_act must refuse with AOG_ERR_UNSUPPORTED: one past the two largest cases, and the widest the dimension check lets through
UNSUPPORTED = [(1024, 497), (4, 849), (4, 1024)]
# cases whose mean is held to F32_SPREAD_FACTOR x the float32 evaluation's spread instead of MEAN_RTOL / MEAN_ATOL (see the GPU test's docstring)
F32_SPREAD_CASES = ()
COV_VAR = 0.5
N_CALLS = 3
OU = dict(mu=0.1, theta=0.3, sigma=0.05)


def case_weights(case, identity=False):
    """float32 (w1, b1, w2, b2, w3, b3, wo, bo) of a case, make_actor's initialisation ranges (U(+-1/sqrt(fan_in)) hidden, U(+-3e-3) output)
    with the output layer scaled by case.out_scale so that the means are of order 1.  identity=True: layers 2 and 3 the identity and the
    output layer the first A rows of the identity, without biases (the zero-pattern construction)."""
    rng = np.random.RandomState(1000 + case.wseed)
    S, H, A = case.S, case.H, case.A
    out = []
    for fan_in, fan_out in ((S, H), (H, H), (H, H)):
        b = 1.0 / math.sqrt(fan_in)
        out += [rng.uniform(-b, b, (fan_out, fan_in)).astype(np.float32), rng.uniform(-b, b, fan_out).astype(np.float32)]
    out += [(rng.uniform(-3e-3, 3e-3, (A, H)) * case.out_scale).astype(np.float32), (rng.uniform(-3e-3, 3e-3, A) * case.out_scale).astype(np.float32)]
    if identity:
        assert A <= H
        eye = np.eye(H, dtype=np.float32)
        out[2:] = [eye, np.zeros(H, np.float32), eye.copy(), np.zeros(H, np.float32), eye[:A].copy(), np.zeros(A, np.float32)]
    return out


def case_obs(case, f16):
    """Observations of a case, uniform in [0, 3) like the existing actor test's: float32, or those rounded to float16."""
    obs = (np.random.RandomState(2000 + case.wseed).random_sample((case.B, case.S)) * 3).astype(np.float32)
    return obs.astype(np.float16) if f16 else obs


def case_ou_start(case):
    """A nonzero float64 OU start state [B, A]."""
    return 0.2 * np.random.RandomState(3000 + case.wseed).randn(case.B, case.A)


def case_query(case, weights, obs, call, keying=KEYING, **kw):
    """reference_query of call number ``call`` (0 .. N_CALLS - 1) of a case."""
    return reference_query(weights, obs, case.p, COV_VAR, case.seed, case.call_index + call, case.env_id_base, keying=keying, **kw)
