"""The checkpoint contract of ``get_state`` / ``set_state`` as one procedure (``resume_case``): a run is interrupted at a snapshot, and
whatever is restored from it — a fresh env built with the same arguments, or the same env after it has moved on — must reproduce the
uninterrupted run bit for bit.  Plain Python: the cases live in test_gpu_checkpoint.py.

A case gives ``make()`` (a new env, or any object with ``get_state`` / ``set_state`` / ``get_screens`` / ``close`` and the counters below) and
``drive(env, n)``, which steps it ``n`` times and returns, per step, the list of CPU numpy copies of everything the case produced in it.  A
drive takes its decisions from the env's restored state alone (``env.timestep``: the actions of ``actions_at``, the resets of
``drive_with``), so that a resumed env is driven exactly like the uninterrupted one."""
import numpy as np

COUNTERS = ("timestep", "episode_no", "observation_frames", "pyramid_frame_count")


def cpu(x):
    """A CPU numpy copy of a device tensor, a numpy array or a number."""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy().copy()
    return np.array(x)


def actions_at(env, scale=0.5):
    """The [B, A] float32 actions of the env's step ``env.timestep``: a function of the restored clock, whoever steps."""
    import torch

    a = np.random.RandomState(1000 + int(env.timestep)).randn(env.num_envs, env.num_modes).astype(np.float32) * scale
    return torch.from_numpy(a).to(env.device)


def step_outputs(ret):
    """obs, obs_raw, reward, done, strehl, power of a step tuple."""
    obs, reward, done, _, info = ret
    return [obs, info["obs_raw"], reward, done, info["strehl"], info["power"]]


def drive_with(T, action=None, before=None, after=None):
    """A drive over episodes of ``T`` steps: a whole-batch ``reset`` (recorded: obs and obs_raw) whenever the clock stands at a multiple of
    ``T``, then per step ``before(env)`` (instrument calls at the state the reset or the last step left; returns what to record),
    ``action(env)`` -> (action, what to record; default ``actions_at``), the step (all six outputs recorded) and ``after(env)``."""
    def drive(env, n):
        out = []
        for _ in range(n):
            rec = []
            if env.timestep % T == 0:
                obs, _ = env.reset()
                rec += [cpu(obs), cpu(env.last_obs_raw)]
            if before is not None:
                rec += [cpu(x) for x in before(env)]
            a, more = action(env) if action is not None else (actions_at(env), [])
            rec += [cpu(x) for x in more]
            ret = env.step(a)
            rec += [cpu(x) for x in step_outputs(ret)]
            assert bool(ret[2].all()) == (env.timestep % T == 0), "the drive's episode clock and the env's done flag disagree"
            if after is not None:
                rec += [cpu(x) for x in after(env)]
            out.append(rec)
        return out
    return drive


def blob_bytes(snap):
    """The sizes of every library blob in a snapshot (a dict that may nest others: a layered env's layers, a rig's env), in order."""
    if isinstance(snap, dict):
        return ([int(snap["blob"].numel())] if "blob" in snap else []) + [n for k, v in snap.items() if k != "blob" for n in blob_bytes(v)]
    if isinstance(snap, (list, tuple)):
        return [n for v in snap for n in blob_bytes(v)]
    return []


def assert_same_run(want, got, what):
    """Every recorded array of ``got`` equals ``want``'s (numpy's array equality: exact values, NaN equal to NaN)."""
    assert len(want) == len(got), f"{what}: {len(got)} steps recorded, {len(want)} expected"
    for t, (x, y) in enumerate(zip(want, got)):
        assert len(x) == len(y), f"{what}: step {t} after the snapshot recorded {len(y)} outputs, {len(x)} expected"
        for j, (u, v) in enumerate(zip(x, y)):
            assert u.dtype == v.dtype and u.shape == v.shape, f"{what}: step {t} after the snapshot, output {j}: {v.dtype}{v.shape} for {u.dtype}{u.shape}"
            np.testing.assert_array_equal(v, u, err_msg=f"{what}: step {t} after the snapshot, output {j} differs from the uninterrupted run")


def resume_case(make, drive, k, m, *, make_fresh=None, halves=("fresh", "advanced"), at_snapshot=None, before_restore=None, restore=None):
    """``drive(make(), k)``, the snapshot, ``m`` more steps (the uninterrupted run); then the resumes ``halves`` names:

    fresh      ``(make_fresh or make)()``, ``set_state(snap)``, ``m`` steps;
    advanced   the first env after its ``m`` further steps (and ``before_restore(env)``, which leaves it work pending where the case has
               such work), ``set_state(snap)``, ``m`` steps.

    Each must equal the uninterrupted run in every recorded array, the final ``get_screens()`` and ``COUNTERS``.  ``at_snapshot(env)``
    runs on every env that stands at the snapshot point before it is driven on; ``restore(env, snap)`` replaces the plain
    ``env.set_state(snap)`` of the advanced half.  Returns the number of recorded arrays per run."""
    env = make()
    others = []
    try:
        drive(env, k)
        snap = env.get_state()
        print("state blob bytes:", blob_bytes(snap))
        if at_snapshot is not None:
            at_snapshot(env)
        first = drive(env, m)
        assert len(first) == m and all(len(r) > 0 for r in first)
        end = dict(screens=cpu(env.get_screens()), **{c: getattr(env, c) for c in COUNTERS})

        def check(e, run, what):
            assert_same_run(first, run, what)
            np.testing.assert_array_equal(cpu(e.get_screens()), end["screens"], err_msg=f"{what}: the final screens differ")
            for c in COUNTERS:
                assert getattr(e, c) == end[c], f"{what}: {c} = {getattr(e, c)}, the uninterrupted run ended at {end[c]}"
            if hasattr(e, "device_status"):
                assert e.device_status() == 0

        if "fresh" in halves:
            other = (make_fresh or make)()
            others.append(other)
            other.set_state(snap)
            if at_snapshot is not None:
                at_snapshot(other)
            check(other, drive(other, m), "fresh env")
        if "advanced" in halves:
            if before_restore is not None:
                before_restore(env)
            if restore is not None:
                restore(env, snap)
            else:
                env.set_state(snap)
            if at_snapshot is not None:
                at_snapshot(env)
            check(env, drive(env, m), "advanced env")
        return sum(len(r) for r in first)
    finally:
        for e in [env] + others:
            e.close()
