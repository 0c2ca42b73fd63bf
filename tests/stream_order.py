"""A busy-stream harness for the stream-ordering contract of the device-pointer entry points (include/pann.h: "launched on
`stream`; no sync, no alloc"; DESIGN.md "Stream order").

On an idle device a kernel, memset or copy that the library put on a stream other than the caller's still finishes in time by
luck.  run_behind_delay() takes the luck away: the caller's stream is kept busy by a delay kernel, the real inputs reach their
buffers only AFTER the delay (until then the buffers hold decoys: different but valid inputs), the outputs are filled with
poison after the delay too, and the entry point is called from the host at once.  Whatever the library enqueued elsewhere runs
during the delay: it reads decoys, and what it writes is poisoned again before the rest of the call runs.  Whether the call
came back while the delay was still running says whether it synchronised.

Measured on an MI355X (tests/test_stream_order_gpu.py, all cases, warmed workspaces, four runs, the schedules in which
returned_early is asserted): the host time from "delay enqueued" to "last entry point returned" has a median of 0.14 ms; its
largest value was 0.18 to 0.21 ms in three runs and 9.5 ms in one (a single schedule, batch_search_masked_dev, presumably a
host thread that lost its CPU: the same case stayed under 0.21 ms in the other runs).  HOST_MS_MEASURED is that largest value; DELAY_MS is at least
20 times it and not below 20 ms, so that a host thread descheduled for a few milliseconds does not fail an assertion of
`returned_early`.  The test module prints the figures of its run (pytest -s).
"""
import time

HOST_MS_MEASURED = 9.5     # ms, see the docstring
DELAY_MS = 200.0
PROBE_MS = 10.0            # independent_streams: long against the two enqueues it has to outlast
POISON_BYTE = 0xA5
POISON_U32 = 0xA5A5A5A5

HOST_MS = []               # one entry per run_behind_delay: delay enqueued -> last call returned (what HOST_MS_MEASURED bounds)
_cycles_per_ms = {}


def _busy(stream, amount):
    """the raw delay kernel: torch.cuda._sleep(cycles), or a chain of large matrix products where torch has none"""
    import torch
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(amount))
        else:
            a = _busy.mat.setdefault(stream.device, torch.ones((2048, 2048), device=stream.device))
            for _ in range(int(amount)):
                torch.mm(a, a)


_busy.mat = {}


def _calibrate(stream):
    """units of _busy per millisecond on this device, measured once per process with two events"""
    import torch
    dev = stream.device
    if dev not in _cycles_per_ms:
        unit = 2_000_000 if hasattr(torch.cuda, "_sleep") else 8
        _busy(stream, unit)                                     # first launch: module load, not timed
        with torch.cuda.stream(stream):                         # ... and the harness's own fill and copy kernels
            warm = torch.zeros(64, dtype=torch.int32, device=dev)
            poison(warm)
            warm.copy_(torch.ones(64, dtype=torch.int32, device=dev))
        stream.synchronize()
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _busy(stream, unit)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        _cycles_per_ms[dev] = unit / max(best, 1e-3)
    return _cycles_per_ms[dev]


def delay(stream, ms):
    """keep `stream` busy for about `ms` milliseconds; nothing else"""
    per_ms = _calibrate(stream)
    _busy(stream, max(1, int(per_ms * ms)))


def poison(t):
    """0xA5 in every byte of tensor t, on the current stream (ids then read 0xA5A5A5A5)"""
    import torch
    t.view(torch.uint8).fill_(POISON_BYTE)


def run_behind_delay(stream, inputs, outputs, calls, ms=None):
    """inputs: (buffer, real) pairs of device tensors of one shape and dtype -- `buffer` is what the entry point is given and
    holds a DECOY now, `real` is the staged real input; outputs: device tensors the entry point writes; calls: callables that
    enqueue the entry point(s) on `stream`.  The schedule, on `stream` alone:

        delay | event | real -> buffer for every input | poison every output | calls() ... | returned_early? | synchronize

    Returns returned_early: the delay was still running when the last call came back to the host."""
    import torch
    ms = DELAY_MS if ms is None else ms
    _calibrate(stream)
    with torch.cuda.stream(stream):
        for o in outputs:
            poison(o)
    torch.cuda.synchronize(stream.device)                      # decoys, staged inputs and poison are all in place
    e_delay = torch.cuda.Event()
    delay(stream, ms)
    t0 = time.perf_counter()
    e_delay.record(stream)
    with torch.cuda.stream(stream):
        for buf, real in inputs:
            assert buf.shape == real.shape and buf.dtype == real.dtype and buf.data_ptr() != real.data_ptr()
            buf.copy_(real)
        for o in outputs:
            poison(o)
    for call in calls:
        call()
    returned_early = not e_delay.query()
    HOST_MS.append((time.perf_counter() - t0) * 1e3)
    stream.synchronize()
    return returned_early


def _overtakes(other, s, probe):
    """does work enqueued on `other` run while `s` sits behind a delay?  s: delay, then flag := 1; other: a copy of flag, enqueued
    at once.  The copy sees the stale 0 iff `other` ran ahead of `s`."""
    import torch
    flag, one, seen = probe
    flag.zero_()
    seen.fill_(7)
    torch.cuda.synchronize(s.device)
    delay(s, PROBE_MS)
    with torch.cuda.stream(s):
        flag.copy_(one)
    with torch.cuda.stream(other):
        seen.copy_(flag)
    torch.cuda.synchronize(s.device)
    return int(seen.cpu()[0]) == 0


def independent_streams(dev, want=2, tries=8):
    """`want` side streams of torch's pool that really overtake each other, and that the null stream overtakes, on this
    machine -- or fewer if the pool's first `tries` streams do not hold that many.  Two HIP streams that share a hardware
    queue run in submission order, which would hide exactly the bug the harness looks for; the probe is the harness's own
    schedule in miniature (delay + late D2D copy on one stream, an unsynchronised reader on the other)."""
    import torch
    dev = torch.device(dev)
    probe = (torch.zeros(64, dtype=torch.int32, device=dev), torch.ones(64, dtype=torch.int32, device=dev),
             torch.zeros(64, dtype=torch.int32, device=dev))
    null = torch.cuda.default_stream(dev)
    pool = [torch.cuda.Stream(device=dev) for _ in range(tries)]
    ok = [s for s in pool if s.cuda_stream != 0 and _overtakes(null, s, probe)]
    chosen = []
    for s in ok:
        if all(_overtakes(s, c, probe) and _overtakes(c, s, probe) for c in chosen):
            chosen.append(s)
            if len(chosen) == want:
                break
    return chosen
