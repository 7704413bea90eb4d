"""A stream that is held busy for a bounded time, for the tests of stream order (tests/test_gpu_stream_order.py).

hold(stream, ms) puts ONE kernel on `stream` that spins for about `ms` milliseconds and ends by itself, and returns an event
recorded right behind it: whatever is enqueued on the stream afterwards cannot start before the event, and
still_held(event) tells whether the kernel is still running.  Nothing here waits for the host: no flag that somebody
releases, no event that is never recorded.  A hold is at most MAX_HOLD_MS long.

The kernel is torch.cuda._sleep (a loop on the device's clock), calibrated once per process the way PyTorch's own stream
tests calibrate it.  Where the calibration shows that it does not hold a stream (a clock that does not tick as the loop
expects), the hold is a chain of square matrix products sized from the same calibration: bounded as well.

Scenario: the library's kernels are launched behind torch's back, so the caching allocator does not know that they still
read a tensor; a tensor dropped while the stream is held could be handed out again under them.  A Scenario keeps every
tensor of a test alive until its final synchronise.
"""
import statistics

MAX_HOLD_MS = 500.0
CAL_CYCLES = 1_000_000   # the fixed count the calibration times
MIN_CAL_MS = 0.05        # 1e6 cycles in less than this would be a 20 GHz clock: _sleep does not hold the stream
MM_N = 2048              # the fallback's matrix size

_cal = None              # ("sleep", cycles per ms) or ("mm", ms per product, (a, b, out))


def _time_ms(stream, work):
    """Milliseconds `work()` takes on `stream` between two events: the median of three runs after one that warms up."""
    import torch
    times = []
    with torch.cuda.stream(stream):
        for i in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            work()
            e1.record(stream)
            e1.synchronize()
            if i:
                times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def _calibrate():
    global _cal
    if _cal is None:
        import torch
        stream = torch.cuda.current_stream()
        ms = _time_ms(stream, lambda: torch.cuda._sleep(CAL_CYCLES))
        if ms >= MIN_CAL_MS:
            _cal = ("sleep", CAL_CYCLES / ms)
        else:
            a = torch.ones((MM_N, MM_N), dtype=torch.float32, device="cuda")
            b, out = a.clone(), torch.empty_like(a)
            _cal = ("mm", _time_ms(stream, lambda: torch.mm(a, b, out=out)), (a, b, out))
    return _cal


def cycles_per_ms():
    """Cycles of torch.cuda._sleep per millisecond on this device (None where the fallback is in use)."""
    cal = _calibrate()
    return cal[1] if cal[0] == "sleep" else None


def method():
    """'sleep' or 'mm': what a hold is made of in this process."""
    return _calibrate()[0]


def hold(stream, ms):
    """Keep `stream` busy for about `ms` milliseconds (at most MAX_HOLD_MS) from now on; returns the event behind the hold."""
    import torch
    ms = min(float(ms), MAX_HOLD_MS)
    cal = _calibrate()
    event = torch.cuda.Event()
    with torch.cuda.stream(stream):
        if cal[0] == "sleep":
            torch.cuda._sleep(max(1, int(ms * cal[1])))
        else:
            a, b, out = cal[2]
            for _ in range(max(1, int(ms / cal[1] + 0.5))):
                torch.mm(a, b, out=out)
        event.record(stream)
    return event


def still_held(event):
    return not event.query()


def hold_ms(t_host_s):
    """The hold of a held pass whose enqueue sequence took t_host_s seconds of host time on an idle device: twenty times that
    (host times on a shared machine jitter several-fold), at least 30 ms, at most MAX_HOLD_MS."""
    return min(MAX_HOLD_MS, max(30.0, 20.0 * 1e3 * t_host_s))


class Scenario:
    """Keeps every tensor of a scenario referenced until the final synchronise."""

    def __init__(self):
        self._kept = []

    def keep(self, *things):
        self._kept.extend(things)
        return things[0] if len(things) == 1 else things

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.synchronize()  # (also on an exception: nothing may still run on what is dropped below)
        self._kept.clear()
        return False
