"""The link telemetry on the device against its numpy restatement (tests/link_reference.py): known float32 sequences are pushed, the
chronological window is taken back out of the state blob, and every output of one statistics call is held to the restatement of that
window — the integers exactly, the float64 sums to the worst case of any summation order."""
import numpy as np
import pytest

import link_reference as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BIG = dict(thresholds_db=np.linspace(-15.0, -0.5, 16), hist_edges_db=np.linspace(-20.0, 6.0, 64), q=np.linspace(1.0, 8.0, 8))   # K = 16, E = 64, Q = 8
SMALL = dict(thresholds_db=[-3.0], hist_edges_db=[-1.0], q=[])                                                                  # K = 1, E = 1, Q = 0
LEVEL = 2.0e-4   # the sequences' median power


def _torch():
    import torch

    return torch


def _background(rng, n, sigma=0.25):
    """A lognormal background around LEVEL, held below 2.2 LEVEL (the bit-error rate's bound on p / P needs a bounded sample)."""
    return np.minimum(LEVEL * np.exp(sigma * rng.randn(n)), 2.2 * LEVEL).astype(np.float32)


def _fade(p, a, b, depth=0.04):
    p[a:b] *= np.float32(depth)


def _short_sequences():
    """length 64: per-env counts 0, 1, 37, 64 and 64 + 29 over two batches of three; in the wrapped env (samples 29 .. 92 remain, the ring's
    physical wrap lies between samples 63 and 64) one fade straddles the wrap and one touches each end of the window."""
    rng = np.random.RandomState(5)
    seqs = {c: _background(rng, c) for c in (0, 1, 37, 64, 93)}
    _fade(seqs[37], 0, 3)
    _fade(seqs[37], 20, 21)
    _fade(seqs[64], 10, 30)
    _fade(seqs[64], 60, 64)
    _fade(seqs[93], 29, 32)
    _fade(seqs[93], 58, 70)
    _fade(seqs[93], 91, 93)
    return [[seqs[0], seqs[1], seqs[37]], [seqs[64], seqs[93], seqs[37]]]


def _long_sequences():
    """length 4096 filled exactly (a lane's chunk is 64 samples): a 200-frame fade over whole chunks, runs that begin or end exactly on chunk
    boundaries, one that is exactly a chunk, one across a boundary, one at each end of the window; a second env with random fades; a plain one."""
    rng = np.random.RandomState(6)
    a, b, c = (_background(rng, 4096) for _ in range(3))
    for lo, hi in ((0, 5), (1000, 1200), (2048, 2058), (2105, 2112), (2560, 2624), (3130, 3140), (4090, 4096)):
        _fade(a, lo, hi)
    for lo in rng.randint(0, 4000, 25):
        _fade(b, lo, lo + rng.randint(1, 60), depth=0.2)
    return [[a, b, c]]


def _push_all(tel, seqs):
    """Sample t of every env that still has one, through masked pushes."""
    torch = _torch()
    B, steps = len(seqs), max(len(s) for s in seqs)
    host = np.zeros((steps, B), dtype=np.float32)
    mask = np.zeros((steps, B), dtype=bool)
    for b, s in enumerate(seqs):
        host[:len(s), b] = s
        mask[:len(s), b] = True
    dev, mdev = torch.from_numpy(host).cuda(), torch.from_numpy(mask).cuda()
    for t in range(steps):
        tel.push(dev[t], None if mask[t].all() else mdev[t])


def _windows(tel):
    u = tel.unpack()
    rings, counts = u["ring"].cpu().numpy(), u["count"].tolist()
    return [ref.window(r, c) for r, c in zip(rings, counts)]


def _references(windows, reference, call):
    out = [ref.statistics(w, reference, ref.db(call["thresholds_db"]), ref.db(call["hist_edges_db"]), call["q"]) for w in windows]
    for w, s in zip(windows, out):   # conditions on the inputs, from the restatement alone
        margin = ref.edge_margin(w, s)
        print("n", s["samples"], "smallest relative distance sample-edge", margin)
        assert margin > 1e-9, "a sample lies too close to an edge: a last-bit difference in the mean could move an integer"
        if s["samples"] and len(call["q"]):
            assert max(call["q"]) <= 8.0 and s["maximum"] / s["reference"] <= 3.0
    return out


def _same(a, b):
    """Two statistics dicts bit for bit, a NaN equal to a NaN."""
    torch = _torch()

    def same(x, y):
        if not x.dtype.is_floating_point:
            return torch.equal(x, y)
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))

    return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)


def _compare(got, want, b, exact_reference):
    """Row b of a statistics dict against the restatement of that env's window."""
    n = want["samples"]
    g = {k: v[b].cpu().numpy() for k, v in got.items()}
    assert int(g["samples"]) == n
    for k in ("below", "fades", "hist"):
        assert g[k].tolist() == want[k], (k, g[k].tolist(), want[k])
    assert g["longest_fade"].tolist() == want["longest"]
    assert int(g["hist"].sum()) == n
    if n == 0:
        for k in ("mean", "mean_square", "scintillation_index", "minimum", "maximum", "reference", "ber", "fade_fraction", "mean_fade_duration"):
            assert np.isnan(g[k]).all(), k
        return
    assert g["minimum"] == np.float32(want["minimum"]) and g["maximum"] == np.float32(want["maximum"])
    for k in ("mean", "mean_square"):
        err = abs(float(g[k]) - want[k]) / want[k]
        print(k, "relative error", err, "bound", n * EPS)
        assert err <= n * EPS, k
    if exact_reference:
        assert float(g["reference"]) == want["reference"]
    else:
        assert abs(float(g["reference"]) - want["reference"]) <= n * EPS * want["reference"] and g["reference"] == g["mean"]
    si = want["scintillation_index"]
    print("scintillation index", float(g["scintillation_index"]), "error", abs(float(g["scintillation_index"]) - si), "bound", 4 * n * EPS * (1 + si))
    assert abs(float(g["scintillation_index"]) - si) <= 4 * n * EPS * (1 + si)
    if want["ber"]:
        err = np.abs(g["ber"] - np.array(want["ber"])) / np.array(want["ber"])
        print("ber relative error", err.max())
        assert err.max() <= 1e-11
    # the derived fields
    below, fades = np.array(want["below"], dtype=np.float64), np.array(want["fades"], dtype=np.float64)
    np.testing.assert_array_equal(g["fade_fraction"], below / n)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(g["mean_fade_duration"], np.where(fades > 0, below / fades, np.nan))
    np.testing.assert_allclose(g["hist_edges"], want["hist_edges"], rtol=4 * n * EPS)


@pytest.fixture(scope="module")
def filled():
    """Every batch pushed once: (telemetry, windows) per batch, shared by the tests below and left unchanged by them."""
    from adaptive_optics_gym_amd import LinkTelemetry

    out = []
    for length, batches in ((64, _short_sequences()), (4096, _long_sequences())):
        for seqs in batches:
            tel = LinkTelemetry(3, length=length, device="cuda:0")
            _push_all(tel, seqs)
            wins = _windows(tel)
            for w, s in zip(wins, seqs):   # the window is what was pushed, the last `length` of it
                assert np.array_equal(w, s[-length:] if len(s) else s)
            out.append((tel, wins))
    yield out
    for tel, _ in out:
        tel.close()


@pytest.mark.parametrize("reference", ["mean", 0.9 * LEVEL])
@pytest.mark.parametrize("call", [BIG, SMALL], ids=["K16-E64-Q8", "K1-E1-Q0"])
def test_statistics_match_the_restatement(filled, call, reference):
    torch = _torch()
    for tel, wins in filled:
        want = _references(wins, reference, call)
        got = tel.statistics(reference=reference, **call)
        for b in range(3):
            _compare(got, want[b], b, exact_reference=reference != "mean")
        # a mask that leaves env 1 out: its rows read NaN / 0, the others keep their bits
        part = tel.statistics(reference=reference, mask=torch.tensor([True, False, True]), **call)
        assert _same({k: v[[0, 2]] for k, v in part.items()}, {k: v[[0, 2]] for k, v in got.items()})
        for k, v in part.items():
            assert bool(torch.isnan(v[1]).all()) if v.dtype.is_floating_point else not bool(v[1].any()), k


def test_the_wrapped_fade_and_the_long_fade_are_what_they_were_built_as(filled):
    """The restatement's answers for the cases built by hand, so that the comparison above is known to cover them: the run over the ring's
    physical wrap is one run of 12, the 200-frame fade one run of 200."""
    wrapped, long = filled[1][1][1], filled[2][1][0]
    s = ref.statistics(wrapped, LEVEL, ref.db([-6.0]))
    assert (s["samples"], s["below"], s["fades"], s["longest"]) == (64, [3 + 12 + 2], [3], [12])
    s = ref.statistics(long, LEVEL, ref.db([-6.0]))
    assert (s["below"], s["fades"], s["longest"]) == ([5 + 200 + 10 + 7 + 64 + 10 + 6], [7], [200])
    got = filled[2][0].statistics(thresholds_db=[-6.0], reference=LEVEL)
    assert (int(got["below"][0, 0]), int(got["fades"][0, 0]), int(got["longest_fade"][0, 0])) == (302, 7, 200)
    assert abs(float(got["mean_fade_duration"][0, 0]) - 302 / 7) < 1e-12


def test_a_non_finite_push_is_skipped_and_reset_empties_only_the_masked_envs():
    torch = _torch()
    from adaptive_optics_gym_amd import LinkTelemetry

    tel, host = LinkTelemetry(3, length=64, device="cuda:0"), ref.RingReference(3, 64)
    rng = np.random.RandomState(8)
    for t in range(70):
        p = _background(rng, 3)
        if t == 5:
            p[1] = np.inf
        if t == 9:
            p[2] = np.nan
        if t == 11:
            p[0] = -np.inf
        mask = None if t % 3 else [True, t % 2 == 0, True]
        tel.push(torch.from_numpy(p).cuda(), None if mask is None else torch.tensor(mask))
        host.push(p, mask)
    u = tel.unpack()
    assert u["count"].tolist() == list(host.count) and u["skipped"].tolist() == list(host.skipped) == [1, 1, 1]
    assert np.array_equal(u["ring"].cpu().numpy(), host.ring)
    before = tel.statistics()
    tel.reset(torch.tensor([False, True, False]))
    host.reset([False, True, False])
    u = tel.unpack()
    assert u["count"].tolist() == list(host.count) and u["skipped"].tolist() == [1, 0, 1] and np.array_equal(u["ring"].cpu().numpy(), host.ring)
    after = tel.statistics()
    assert int(after["samples"][1]) == 0 and bool(torch.isnan(after["mean"][1])) and not bool(after["hist"][1].any())
    for k in ("mean", "mean_square", "below", "fades", "hist"):
        assert torch.equal(after[k][[0, 2]], before[k][[0, 2]]), k
    tel.reset()
    assert tel.unpack()["count"].tolist() == [0, 0, 0] and tel.statistics()["samples"].tolist() == [0, 0, 0]
    tel.close()


def test_state_round_trips_and_a_split_batch_reproduces_the_whole(filled):
    torch = _torch()
    from adaptive_optics_gym_amd import LinkTelemetry

    for tel, _ in filled[1:]:      # the wrapped batch of length 64 and the filled one of length 4096
        want = tel.statistics(reference="mean", **BIG)
        blob = tel.get_state()
        assert blob.dtype == torch.uint8 and blob.numel() == tel.state_bytes() == 3 * (4 * tel.length + 16)
        twin = LinkTelemetry(3, length=tel.length, device="cuda:0")
        twin.set_state(blob)
        assert torch.equal(twin.get_state(), blob) and _same(twin.statistics(reference="mean", **BIG), want)
        other = LinkTelemetry(3, length=tel.length, device="cuda:0")
        other.load_state_dict(tel.state_dict())
        assert _same(other.statistics(reference="mean", **BIG), want)
        with pytest.raises(ValueError, match="length"):
            LinkTelemetry(3, length=128, device="cuda:0").load_state_dict(tel.state_dict())
        with pytest.raises(ValueError, match="link telemetry"):
            other.set_state(blob[:-1])
        # envs [0, 2) and [2, 3) in two instances: the blob of the whole is the blobs of its parts in a row
        rec = 4 * tel.length + 16
        first, second = LinkTelemetry(2, length=tel.length, device="cuda:0"), LinkTelemetry(1, length=tel.length, device="cuda:0", global_env_offset=2)
        first.set_state(blob[:2 * rec])
        second.set_state(blob[2 * rec:])
        for reference in ("mean", 0.9 * LEVEL):
            whole = tel.statistics(reference=reference, **BIG)
            a, b = first.statistics(reference=reference, **BIG), second.statistics(reference=reference, **BIG)
            assert _same({k: torch.cat([a[k], b[k]]) for k in whole}, whole)
        for t in (twin, other, first, second):
            t.close()


def test_a_split_batch_of_the_same_pushes_reproduces_the_whole():
    torch = _torch()
    from adaptive_optics_gym_amd import LinkTelemetry

    whole, first, second = (LinkTelemetry(n, length=64, device="cuda:0") for n in (3, 2, 1))
    rng = np.random.RandomState(9)
    for t in range(93):
        p = torch.from_numpy(_background(rng, 3) * np.float32(0.05 if 40 <= t < 52 else 1.0)).cuda()
        whole.push(p)
        first.push(p[:2].contiguous())
        second.push(p[2:].contiguous())
    w, a, b = (t.statistics(reference="mean", **BIG) for t in (whole, first, second))
    assert _same({k: torch.cat([a[k], b[k]]) for k in w}, w) and int(w["fades"].sum()) > 0
    for t in (whole, first, second):
        t.close()


ENV_KW = dict(atm_type="dynamic", atm_vel=20.0, SH_operation=True, act_dim=8, obs_dim=2, num_pupil_pixels=32, rew_type="strehl_ratio", seed=23,
              verbose=False)


def test_rollout_feeds_the_link_and_leaves_the_transitions_alone():
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv, LinkTelemetry
    from adaptive_optics_gym_amd.rollout import rollout

    B, T, E = 2, 5, 2
    env, twin = (BatchedAOEnv(B, "cuda:0", timesteps_per_episode=T, **ENV_KW) for _ in range(2))
    tel = LinkTelemetry(B, length=64, device=env.device)
    powers, inner = [], env.step

    def step(actions, out=None):
        ret = inner(actions, out=out)
        powers.append(ret[4]["power"].clone())
        return ret

    env.step = step
    try:
        got = rollout(env, None, episodes=E, policy="ideal", link=tel)
        want = rollout(twin, None, episodes=E, policy="ideal")
        for k in ("obs", "act", "log_prob", "rew", "next_obs", "done", "ep_returns"):
            assert torch.equal(got[k], want[k]), k
        u = tel.unpack()
        assert u["count"].tolist() == [T * E] * B and u["skipped"].tolist() == [0] * B and len(powers) == T * E
        assert torch.equal(u["ring"][:, :T * E], torch.stack(powers, dim=1)) and float(u["ring"][:, :T * E].min()) > 0
        for w, ring in zip(tel.window(), u["ring"]):
            assert torch.equal(w, ring[:T * E])
        s = tel.statistics()
        assert s["samples"].tolist() == [T * E] * B and bool(torch.isfinite(s["scintillation_index"]).all())
        with pytest.raises(ValueError, match="link holds 3 envs"):
            rollout(env, None, episodes=1, policy="ideal", link=LinkTelemetry(3, length=64, device=env.device))
        assert tel.unpack()["count"].tolist() == [T * E] * B      # (refused before the first step)
    finally:
        tel.close()
        env.close()
        twin.close()
