"""Delayed-producer harness of ``test_gpu_streams.py`` (a helper: nothing here is collected).

Every library call takes the caller's stream.  On the legacy default stream every blocking copy, null-stream fill and launch is ordered
implicitly, so an ordering mistake cannot show there.  Here a script of calls runs twice, on two handles built alike:

* the twin: every call on the default stream (``Runner(torch)``), which the oracle tests already hold;
* the run under test: every call on a side stream made by ``torch.cuda.Stream()`` (non-blocking: ``stream_flags`` asks the HIP runtime
  that torch has loaded through ``hipStreamGetFlags``; when the symbol cannot be reached it returns None and the check is left out).

Before a call, each of its input tensors (``Runner.input``) holds a sentinel (NaN; a mask holds its complement) and the device is idle.
On the side stream the runner then enqueues a delay (``torch.cuda._sleep``), the copies that bring the real values, an event, the call
itself and a clone of everything it returned.  Work of the call that is not ordered behind the caller's stream (a launch or a copy on
another stream, a blocking upload) runs during the delay, on the sentinels or on the state before them, and the results differ from the
twin's: a deterministic wrong answer where the default stream would hide a race.  Right after the call returns on the host the event
must not have fired (``queued``): the call was enqueued while its inputs still held the sentinels, so a delay that is too short fails
instead of passing vacuously.  The calls of ``BLOCKING_BY_CONTRACT`` are exempt from that one assertion.  Nothing touches the default
stream between the producer and the side stream's synchronise.

A side stream is used only after ``side_stream`` has shown that it runs beside the null stream.  The runtime spreads its streams over a few
hardware queues (4 by default), and a side stream that shares the null stream's queue is serialised with it in hardware: work that a
mistake puts on the null stream would then wait behind the delay by accident and the mistake would not show.  The probe enqueues a
delay on the candidate, then a trivial operation on the null stream, and takes the candidate only if the null stream's operation has
finished while the candidate's delay is still running; otherwise it draws the next stream.

What the harness cannot show: a zero-fill on the null stream that is still running when the first kernel on the caller's stream starts
(the delay gives such a fill time to finish).  The library does not leave that to chance: ``dev_alloc_bytes`` waits for its fill.

A call that blocks (``BLOCKING_BY_CONTRACT``) drains the delay: what the same ``fn`` group enqueues after it is compared with the twin like
everything else but no longer runs behind the producer.  Groups put the blocking call last, or directly in front of the call that reads
what it wrote.

Results are compared bit for bit, a NaN equal to a NaN (as ``test_gpu_link._same``); ``rtol`` names the project's stated exceptions.
"""
import ctypes
import re
import time

import numpy as np

# Calls that synchronise by contract: exempt from the `queued` self-check, and only from it.  Each with the line that says it blocks.
BLOCKING_BY_CONTRACT = {
    "get_state": "batched_env.py get_state: synchronises the stream after aog_get_state; aogym.hip aog_get_state: hipStreamSynchronize before the "
                 "blocking copy of the tail",
    "set_state": "batched_env.py set_state / device_handle.py set_state: synchronise ('b may be a temporary'); aogym.hip aog_set_state: "
                 "hipStreamSynchronize before reading the tail",
    "device_status": "batched_env.py device_status: 'Synchronise and return the library's sticky device status word'",
    "device_bytes": "batched_env.py device_bytes: aog_get_info, a host query",
    "spgd_set_params": "sensorless.py set_params: synchronises first ('the copy is blocking but not ordered behind this stream's queries')",
    "set_screens": "batched_env.py set_screens: 'the kernel is stream-ordered; keep the source alive until it has run', then synchronises",
    "set_actuators": "batched_env.py set_actuators: synchronises the stream after aog_set_actuators",
    "sh_update": "batched_env.py sh_update: synchronises the stream after aog_sh_update",
    "unpack": "device_handle.py get_state then host-side views: LinkTelemetry.window copies the counts to the host",
    "rollout": "rollout.py rollout: returns avg_ep_rew as a Python float (a host copy of the episode returns)",
    "pyramid_calibrate": "batched_env.py pyramid_calibrate / PYR_step (first call): builds a scratch env and copies its slopes to the host",
    "host_copy": "link.py statistics (hist_edges: torch.as_tensor of a host array on the device), batched_env.py _instrument_mask and reset(mask) with "
                 "a host mask (the mask goes from host memory to the device): torch copies pageable host memory to the device synchronously",
    "lazy_create": "link.hip aog_link_create / telemetry.hip aog_telemetry_create: a reset kernel on the null stream, then "
                   "hipStreamSynchronize(nullptr); LinkTelemetry and ModalTelemetry make their handle in the first call (lazy = True)",
    "upload": "science.hip aog_upload_science / pyramid.hip aog_upload_pyramid: hipDeviceSynchronize ('a camera uploaded before may still be "
              "integrating into the buffers given back here'); focal.hip mft_work_alloc (line 44): hipDeviceSynchronize after the first "
              "focal_images has allocated and filled its work grid on the null stream",
    "screen_workspace": "screens.hip: hipDeviceSynchronize before a synthesis workspace or plan is replaced",
}

FLOOR_MS = 40.0    # the delay per library call behind a producer, at the least (Runner.call)


def _hip():
    """The HIP runtime torch has loaded, as a ctypes library (None when it cannot be found)."""
    names = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    names.append(line.split()[-1])
                    break
    except OSError:
        pass
    for name in names + ["libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"]:
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    return None


def stream_flags(stream):
    """hipStreamGetFlags of a torch stream (hipStreamNonBlocking = 1), or None when the runtime's symbol is not reachable."""
    lib = _hip()
    if lib is None or not hasattr(lib, "hipStreamGetFlags"):
        return None
    flags = ctypes.c_uint(0)
    rc = lib.hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags))
    return int(flags.value) if rc == 0 else None


def calibrate(torch):
    """Cycles of torch.cuda._sleep per millisecond, measured with two events on a side stream (second of two runs)."""
    s = torch.cuda.Stream()
    ms = 0.0
    cycles = 20_000_000
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        s.synchronize()
        ms = e0.elapsed_time(e1)
    assert ms > 0.5, f"torch.cuda._sleep({cycles}) took {ms} ms: it does not delay the stream on this device"
    return cycles / ms


def runs_beside_null_stream(torch, stream, cycles_per_ms, ms=5.0):
    """True when an operation on the null stream finishes while a delay on ``stream`` is still running: the two do not share a hardware queue
    (and ``stream`` is non-blocking).  The device is idle before and after."""
    probe = torch.zeros((1,), device="cuda")
    null = torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles_per_ms * ms))
        side_ev = torch.cuda.Event()
        side_ev.record(stream)
    with torch.cuda.stream(null):
        probe.add_(1)
        null_ev = torch.cuda.Event()
        null_ev.record(null)
    null_ev.synchronize()
    beside = not side_ev.query()
    torch.cuda.synchronize()
    return beside


_REJECTED = []   # streams the probe turned down stay alive, so that the next draw is another one


def side_stream(torch, cycles_per_ms, tries=16):
    """A new ``torch.cuda.Stream()`` that is shown to run beside the null stream (AssertionError when ``tries`` draws give none)."""
    for _ in range(tries):
        s = torch.cuda.Stream()
        flags = stream_flags(s)
        assert flags is None or flags & 1, "torch.cuda.Stream() is not non-blocking: the side stream would wait for the null stream"
        if all(runs_beside_null_stream(torch, s, cycles_per_ms) for _ in range(2)):
            return s
        _REJECTED.append(s)
    raise AssertionError(f"none of {tries} side streams ran beside the null stream: the delayed producer could not show a null-stream mistake")


def _clone(torch, x):
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, dict):
        return {k: _clone(torch, v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_clone(torch, v) for v in x]
    if isinstance(x, np.ndarray):
        return x.copy()
    return x


def _flatten(torch, x, path, out):
    if isinstance(x, dict):
        for k in x:
            _flatten(torch, x[k], f"{path}.{k}", out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flatten(torch, v, f"{path}[{i}]", out)
    else:
        out.append((path, x))


def same(torch, a, b, rtol=None):
    """Bit for bit, a NaN equal to a NaN; with ``rtol``: to that relative tolerance of the twin's value, NaNs still in the same places."""
    if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
        return False
    if not isinstance(a, torch.Tensor):
        if isinstance(a, np.ndarray):
            return isinstance(b, np.ndarray) and a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
        if isinstance(a, float) and isinstance(b, float) and a != a:
            return b != b
        return type(a) is type(b) and a == b
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    if not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    a, b = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)
    if rtol is None:
        return bool(torch.equal(a, b))
    return bool((a.double() - b.double()).abs().le(rtol * b.double().abs()).all())


class Runner:
    """Runs a script's calls: on the default stream (the twin; ``side`` None) or behind the delayed producer on ``side``."""

    def __init__(self, torch, side=None, cycles_per_ms=0.0, twin=None):
        self.torch, self.side, self.cycles_per_ms, self.twin = torch, side, float(cycles_per_ms), twin
        self.outputs = []      # (label, clone of what the call returned)
        self.chains = []       # twin: per producer [library calls behind it, their host seconds, whether one of them is exempt, first label]
        self.problems = []     # run under test: what the self-check found
        self.delays = []       # run under test: (delay in ms, label) of every producer
        self.tightest = (0.0, "", 0.0, 0.0)   # run under test: (share of the delay used up, label, host ms behind the producer, delay ms)
        self._staged = []
        self._ev = None        # the last producer's event while nothing has drained the stream since
        self._t_ev = self._delay_ms = 0.0
        self._keep = []        # every input lives as long as the runner: nothing goes back to the allocator of another stream

    def input(self, value, dtype=None):
        """A device tensor for the NEXT call: it holds a sentinel now and ``value`` only once that call's producer has run."""
        torch = self.torch
        src = torch.as_tensor(np.asarray(value) if not isinstance(value, torch.Tensor) else value)
        src = src.to("cuda", dtype=dtype).contiguous().clone()
        if src.dtype.is_floating_point:
            dst = torch.full_like(src, float("nan"))
        elif src.dtype == torch.bool:
            dst = ~src
        else:
            dst = src ^ 0x55
        self._staged.append((dst, src))
        self._keep.append((dst, src))
        return dst

    def use(self, stream):
        """Run under test: continue on ``stream`` (from ``side_stream``, or the default stream), which first waits for the stream used so far.
        The twin stays where it is."""
        if self.side is not None:
            stream.wait_stream(self.side)
            self.side = stream

    def call(self, label, fn, blocking=None, lead=True, drain=True, weight=1):
        """``fn()`` is one library call or a group of calls made back to back (``weight``: how many).  ``blocking``: the key of
        BLOCKING_BY_CONTRACT that exempts it from the self-check.  ``lead=False``: no settling, delay or producer in front (the call follows
        the last one directly and shares its producer; it has no inputs of its own, and the self-check asks that the producer is still
        pending after it too); ``drain=False``: the stream is not synchronised afterwards.

        The delay of a producer covers everything behind it: max(FLOOR_MS x the library calls that share it, 10 x the host-side duration
        of those calls and of the producer's copies on the twin)."""
        torch = self.torch
        assert blocking is None or blocking in BLOCKING_BY_CONTRACT, blocking
        staged, self._staged = self._staged, []
        assert lead or not staged, "a call without a producer cannot have delayed inputs"
        if self.side is None:
            t0 = time.perf_counter()   # (the producer's copies count: the run under test enqueues them in front of the call)
            for dst, src in staged:
                dst.copy_(src)
            out = fn()
            dt = time.perf_counter() - t0
            if lead:
                self.chains.append([0, 0.0, False, label])
            chain = self.chains[-1]
            chain[0] += int(weight)
            chain[1] += dt
            chain[2] = chain[2] or blocking is not None
            tree = _clone(torch, out)
            torch.cuda.synchronize()
        else:
            if lead:
                torch.cuda.synchronize()   # the sentinels are in place and the device is idle
                n, dt, exempt, first = self.twin.chains[len(self.delays)]
                assert first == label, (first, label)
                self._delay_ms = max(FLOOR_MS * n, 0.0 if exempt else 10e3 * dt)
                self.delays.append((self._delay_ms, label))
            with torch.cuda.stream(self.side):
                queued = True
                if lead:
                    torch.cuda._sleep(int(self.cycles_per_ms * self._delay_ms))
                    for dst, src in staged:
                        dst.copy_(src, non_blocking=True)
                    self._ev = torch.cuda.Event()
                    self._ev.record(self.side)
                    self._t_ev = time.perf_counter()
                out = fn()
                if self._ev is not None:   # (lead=False: the producer of the last leading call, still in front of everything since)
                    queued = not self._ev.query()
                    behind = 1e3 * (time.perf_counter() - self._t_ev)
                    if blocking is None and behind / self._delay_ms > self.tightest[0]:
                        self.tightest = (behind / self._delay_ms, label, behind, self._delay_ms)
                tree = _clone(torch, out)
            if drain:
                self.side.synchronize()
                self._ev = None
            if not queued and blocking is None:
                self.problems.append(f"{label}: the producer had finished when the call returned (it blocked, or the delay is too short)")
        self.outputs.append((label, tree))
        return out

    def longest(self):
        """The twin's longest non-exempt chain of calls behind one producer: (host seconds, first label)."""
        rows = [(dt, label) for _, dt, exempt, label in self.chains if not exempt]
        return max(rows) if rows else (0.0, "")


def compare(torch, twin, run, rtol=None):
    """Every difference between the run under test and the twin, as a list of lines (empty: the same bits).  ``rtol``: {a call's
    label, or a dict key inside what a call returned, matched exactly: relative tolerance} for the results the project
    states to be equal to rounding only."""
    torch.cuda.synchronize()
    lines = list(run.problems)
    if [l for l, _ in twin.outputs] != [l for l, _ in run.outputs]:
        return lines + ["the two runs made different calls"]
    for (label, want), (_, got) in zip(twin.outputs, run.outputs):
        fw, fg = [], []
        _flatten(torch, want, label, fw)
        _flatten(torch, got, label, fg)
        if [p for p, _ in fw] != [p for p, _ in fg]:
            lines.append(f"{label}: the results have different structure")
            continue
        for (path, w), (_, g) in zip(fw, fg):
            tol = (rtol or {}).get(label)
            for key in re.findall(r"\.(\w+)", path[len(label):]):
                tol = (rtol or {}).get(key, tol)
            if not same(torch, g, w, tol):
                extra = ""
                if isinstance(g, torch.Tensor) and isinstance(w, torch.Tensor) and g.shape == w.shape:
                    gg = torch.view_as_real(g) if g.is_complex() else g
                    extra = f" ({int(torch.isnan(gg.double()).sum())} NaN of {gg.numel()} values)"
                lines.append(f"{path}: differs from the default-stream twin{extra}")
    return lines
