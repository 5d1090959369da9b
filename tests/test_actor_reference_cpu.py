"""Host-only tests of tests/actor_reference.py, the restatement the GPU tests of the policy query compare against: Philox known answers, the
uniform mappings at their edge words, and — for every case of the GPU table — that the reference ALONE tells the documented keying from each
wrong one by a wide margin, and that the GPU tests' comparison functions reject a wrongly keyed result put in the device's place."""
import numpy as np
import pytest

import actor_reference as ar


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    """Random123's published vectors of Philox4x32-10."""
    assert _hex(philox_scalar(counter, key)) == expect
    # the same through the vectorised path, broadcast beside other counters
    c = [np.array([1, x, 2], dtype=np.uint64) for x in counter]
    out = ar.philox4x32_10(c, key)
    assert _hex([w[1] for w in out]) == expect


def philox_scalar(counter, key):
    return [w.reshape(-1)[0] for w in ar.philox4x32_10([np.array([x]) for x in counter], key)]


EDGE_WORDS = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0xFFFFFF7F, 0xFFFFFFFF], dtype=np.uint32)


def test_uniform_mappings_at_edge_words():
    u = ar.mask_uniform(EDGE_WORDS)
    assert u.dtype == np.float32 and np.all(u >= 0) and np.all(u < 1)
    np.testing.assert_array_equal(u, np.array([0, 0, 2.0 ** -24, (2 ** 23 - 1) * 2.0 ** -24, (2 ** 24 - 1) * 2.0 ** -24, (2 ** 24 - 1) * 2.0 ** -24],
                                              dtype=np.float32))
    # keep iff u >= p: p = 0 keeps everything; 0.5 keeps the upper half (0x7FFFFFFF is just below); 0.9 only the top words
    np.testing.assert_array_equal(ar.keep_mask(EDGE_WORDS, 0.0), [True] * 6)
    np.testing.assert_array_equal(ar.keep_mask(EDGE_WORDS, 0.5), [False, False, False, False, True, True])
    np.testing.assert_array_equal(ar.keep_mask(np.array([0x80000000], dtype=np.uint32), 0.5), [True])
    np.testing.assert_array_equal(ar.keep_mask(EDGE_WORDS, 0.9), [False, False, False, False, True, True])
    assert ar.keep_scale(0.0) == 1 and ar.keep_scale(0.5) == 2 and ar.keep_scale(0.9) == np.float32(1) / (np.float32(1) - np.float32(0.9))
    v = ar.normal_uniform(EDGE_WORDS)
    assert v.dtype == np.float32 and np.all(v > 0) and np.all(v <= 1)
    assert v[0] == np.float32(2.0 ** -33) and v[1] == np.float32(255.5 * 2.0 ** -32) and v[3] == np.float32(0.5)
    # 2^32 - 129 rounds down to 2^32 - 256; the largest word rounds to 2^32, u = exactly 1: kept, log(1) = 0 is a valid radius
    assert v[4] == np.float32(1 - 2.0 ** -24) and v[5] == 1.0
    # every pairing of the edge words gives finite normals, the radius at most sqrt(-2 ln 2^-33) = 6.76
    pairs = np.array([[a, b, b, a] for a in EDGE_WORDS for b in EDGE_WORDS], dtype=np.uint32)
    n = ar.normals(pairs)
    assert np.all(np.isfinite(n)) and float(np.abs(n).max()) <= 6.8
    np.testing.assert_allclose(np.hypot(n[0, 0], n[0, 1]), np.sqrt(66 * np.log(2.0)), rtol=1e-12)


def test_stream_words_layout():
    """The counter layout, word for word, against single Philox calls."""
    seed, call, base = 0x1234567890ABCDEF, (1 << 32) + 7, 12345
    w = ar.stream_words(3, 10, base + np.arange(2), seed, call)
    for row in range(2):
        for m in range(10):
            c = [(m & ~3) | (3 << 24), base + row, call & 0xFFFFFFFF, (call >> 32) ^ 0xAC70]
            assert w[row, m] == philox_scalar(c, (seed & 0xFFFFFFFF, seed >> 32))[m & 3]
    # units past a multiple of four still come from their own group's call: cutting a longer stream gives the shorter one
    np.testing.assert_array_equal(ar.stream_words(4, 6, [7], 1, 2), ar.stream_words(4, 64, [7], 1, 2)[:, :6])
    np.testing.assert_array_equal(ar.stream_normals(4, 6, [7], 1, 2), ar.stream_normals(4, 64, [7], 1, 2)[:, :6])
    # a split batch reproduces the whole one
    np.testing.assert_array_equal(ar.stream_words(1, 9, np.arange(5, 9), 3, 4), ar.stream_words(1, 9, np.arange(9), 3, 4)[5:])


def test_reference_query_forms():
    case = ar.CASES[1]
    w, obs = ar.case_weights(case), ar.case_obs(case, True)
    q = ar.case_query(case, w, obs, 0)
    std = np.sqrt(0.5)
    np.testing.assert_allclose(q.action, q.mean + std * q.eps, rtol=0, atol=1e-15)
    np.testing.assert_allclose(q.log_prob, -0.5 * (q.eps ** 2).sum(1) - 0.5 * case.A * np.log(np.pi), rtol=1e-14)
    qm = ar.case_query(case, w, obs, 0, mode="mean")
    np.testing.assert_array_equal(qm.action, qm.mean)
    np.testing.assert_array_equal(qm.mean, q.mean)
    np.testing.assert_allclose(qm.log_prob, -0.5 * case.A * np.log(np.pi), rtol=1e-14)
    s0 = ar.case_ou_start(case)
    qo = ar.case_query(case, w, obs, 0, ou_state=s0, **ar.OU)
    n = ar.stream_normals(5, case.A, np.arange(case.B), case.seed, case.call_index)
    np.testing.assert_array_equal(qo.ou_state, s0 + (0.3 * (0.1 - s0) + 0.05 * n))
    assert np.max(np.abs(n - q.eps)) > 1          # tag 5 is a stream of its own
    np.testing.assert_array_equal(qo.action, (q.action.astype(np.float32).astype(np.float64) + qo.ou_state).astype(np.float32))
    # with p = 0 the reference is the plain eval-mode forward
    q0 = ar.reference_query(w, obs, 0.0, 0.5, 1, 2)
    x = obs.astype(np.float64)
    for layer in range(3):
        x = np.maximum(x @ w[2 * layer].astype(np.float64).T + w[2 * layer + 1], 0)
    np.testing.assert_array_equal(q0.mean, x @ w[6].astype(np.float64).T + w[7])


def _as_device(q):
    """What a correct device would return for reference result q: float32 mean, action, log_prob."""
    mean = q.mean.astype(np.float32)
    action = (q.mean + ar.device_std(ar.COV_VAR) * q.eps).astype(np.float32)
    return mean, action, q.log_prob.astype(np.float32)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ar.CASES, ids=[c.name for c in ar.CASES])
def test_reference_discriminates_wrong_keyings(case, f16):
    """For every case of the GPU table and each of its three calls: the reference recomputed with each wrong keying moves more than 90 % of
    the means (eps for the variants that touch eps) by more than 100 x the tolerance the GPU test applies, and the GPU test's comparison
    functions reject it where they accept the rightly keyed result rounded to float32.  A condition on the reference alone.

    With dropout_p = 0 every unit is kept whatever the words say, so the masks cannot move the mean: that case is held to the eps variants,
    and its group variant to the eps of the units whose group that variant changes (m & 12 != 0: three quarters of them)."""
    w, obs = ar.case_weights(case), ar.case_obs(case, f16)
    for call in range(ar.N_CALLS):
        q = ar.case_query(case, w, obs, call)
        spread = q.mean_f32_spread if case.name in ar.F32_SPREAD_CASES else None
        mean, action, log_prob = _as_device(q)
        ar.check_mean(mean, q.mean, spread)
        ar.check_eps(action, mean, ar.COV_VAR, q.eps)
        ar.check_log_prob(log_prob, q.log_prob)
        # the next call's stream is not within tolerance of this one's
        assert ar.eps_differs(action, mean, ar.COV_VAR, ar.case_query(case, w, obs, call + 1).eps)
        for name, (keying, moves) in ar.WRONG_KEYINGS.items():
            units = np.ones(case.A, dtype=bool)
            if case.p == 0.0:
                moves = tuple(m for m in moves if m == "eps")
                if name == "unit_group_of_16":
                    moves, units = ("eps",), (np.arange(case.A) & 12) != 0
            bad = ar.case_query(case, w, obs, call, keying=keying)
            b_mean, b_action, b_log_prob = _as_device(bad)
            if "mean" in moves:
                moved = np.abs(bad.mean - q.mean) > 100 * ar.mean_bound(q.mean, spread)
                assert moved.mean() > 0.9, f"{name}, call {call}: only {moved.mean():.3f} of the means move"
                with pytest.raises(AssertionError):
                    ar.check_mean(b_mean, q.mean, spread)
            if "eps" in moves:
                moved = (np.abs(bad.eps - q.eps) > 100 * ar.EPS_TOL)[:, units]
                assert moved.mean() > 0.9, f"{name}, call {call}: only {moved.mean():.3f} of the eps move"
                with pytest.raises(AssertionError):
                    ar.check_eps(b_action, b_mean, ar.COV_VAR, q.eps)
                with pytest.raises(AssertionError):   # the right mean with the wrong eps
                    ar.check_eps((q.mean + ar.device_std(ar.COV_VAR) * bad.eps).astype(np.float32), mean, ar.COV_VAR, q.eps)
    # the OU normals: a wrongly keyed tag-5 stream is rejected by the state comparison
    s0 = ar.case_ou_start(case)
    good = ar.case_query(case, w, obs, 0, ou_state=s0, **ar.OU)
    assert ar.check_ou_state(good.ou_state, good.ou_state, ar.OU["sigma"]) == 0.0
    for name in ("call_index_plus_1", "call_index_plus_2^32", "seed_xor_2^32", "env_id_base_plus_1", "cos_sin_swapped"):
        bad = ar.case_query(case, w, obs, 0, ou_state=s0, keying=ar.WRONG_KEYINGS[name][0], **ar.OU)
        with pytest.raises(AssertionError):
            ar.check_ou_state(bad.ou_state, good.ou_state, ar.OU["sigma"])
    with pytest.raises(AssertionError):   # eps's stream (tag 4) in the place of tag 5
        ar.check_ou_state(s0 + (ar.OU["theta"] * (ar.OU["mu"] - s0) + ar.OU["sigma"] * good.eps), good.ou_state, ar.OU["sigma"])


@pytest.mark.parametrize("case", [c for c in ar.CASES if c.A <= c.H], ids=lambda c: c.name)
def test_zero_pattern_discriminates(case):
    """The identity construction: the must-be-zero / must-be-nonzero sets of the right keying reject a mean computed under each keying that
    moves the masks, and the undecided elements (|pre-activation| within the margin) are few."""
    w, obs = ar.case_weights(case, identity=True), ar.case_obs(case, True)
    q = ar.case_query(case, w, obs, 0)
    zero, nonzero = ar.zero_pattern(w, obs, q.masks)
    ar.check_zero_pattern(q.mean.astype(np.float32), zero, nonzero)
    assert np.mean(~zero & ~nonzero) < 0.01
    if case.p == 0.0:
        assert nonzero.any() and not np.any(~np.stack(q.masks))
        return
    rejected = 0
    for name, (keying, moves) in ar.WRONG_KEYINGS.items():
        if "mean" not in moves:
            continue
        bad = ar.case_query(case, w, obs, 0, keying=keying)
        try:
            ar.check_zero_pattern(bad.mean.astype(np.float32), zero, nonzero)
        except AssertionError:
            rejected += 1
    # tags 2 and 3 swapped leaves this construction's product of masks as it is (that variant is caught by the dense-weight means).  A case
    # with a handful of elements (one env and one unit; 30 elements kept with probability 1e-3) has too few survivors for its pattern to
    # tell keyings apart: there the pattern is one more check of the right keying, no more
    if case.B * case.A >= 500:
        assert rejected >= 5, rejected
