"""What tests/test_gpu_streams.py shares: the delay kernel and its calibration, decoy inputs, and the side-stream run that holds
a call to the three stream checks (late input, null stream, asynchrony).  Host code only; a GPU is needed to call any of it.

The late-input run, for a call f(*inputs) -> outputs on a side stream S:
    f(*decoys) on the default stream (the workspace then holds the decoys' intermediate results)
    buffers <- decoys (on the default stream, then the device is drained)
    under S:  delay;  buffers <- the true inputs (device-to-device copy_);  f(*buffers);  clone the outputs
    S.synchronize()
Whatever f issues on another stream than S — the null stream, a stream of the library's own — runs while the delay holds S back:
it reads the decoys, or writes before the true inputs arrive, and the outputs differ from the default-stream baseline in their bits.
"""
import time

import numpy as np
import torch

DELAY_CAP_MS = 200.0    # no test may hold a card longer than this per delay
DELAY_FLOOR_MS = 20.0   # ... and the delay is never shorter than this, whatever the calls measure
MARGIN = 10.0           # the delay is at least MARGIN x the warm host time of the slowest call held to the asynchrony check
HEADROOM = 1.3          # the cycle count aims this far above the bound, so that the measured delay meets it
PROBE_CYCLES = 2_000_000

ENQUEUES = "enqueues"           # only enqueues work: S is still held by the delay when the call returns
SYNCHRONISES = "synchronises"   # documented to wait for the stream: S is idle when the call returns


class Delay:
    """torch.cuda._sleep(cycles) on the current stream, `cycles` chosen once per session (calibrate)."""

    def __init__(self):
        self.cycles = None
        self.ms = None             # the delay, measured with a pair of events
        self.slowest = (None, 0.)  # (name, warm host ms) of the slowest call timed at calibration
        self.checked = {}          # name -> warm host ms of every call held to the asynchrony check since

    @staticmethod
    def _time(cycles, stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        stream.synchronize()
        return e0.elapsed_time(e1)

    def calibrate(self, warm_calls):
        """warm_calls: {name: callable} — each has run before (its shape is warm); timed on the default stream, host side only."""
        s = torch.cuda.Stream()
        self._time(1000, s)  # (the kernel itself is loaded)
        per_cycle = self._time(PROBE_CYCLES, s) / PROBE_CYCLES
        for name, call in warm_calls.items():
            worst = 0.
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                worst = max(worst, (time.perf_counter() - t0) * 1e3)
            if worst > self.slowest[1]:
                self.slowest = (name, worst)
        torch.cuda.synchronize()
        want = min(DELAY_CAP_MS, HEADROOM * max(DELAY_FLOOR_MS, MARGIN * self.slowest[1]))
        self.cycles = max(1, int(want / per_cycle))
        self.ms = self._time(self.cycles, s)
        print(f"delay: torch.cuda._sleep({self.cycles}) = {self.ms:.1f} ms ({PROBE_CYCLES} cycles = {per_cycle * PROBE_CYCLES:.2f} ms); "
              f"slowest warm host time {self.slowest[1]:.3f} ms ({self.slowest[0]})")
        assert 0.8 * want <= self.ms <= 1.25 * DELAY_CAP_MS, (want, self.ms)  # (_sleep is linear in its cycles, or it is no delay)
        return self

    def __call__(self):
        torch.cuda._sleep(self.cycles)


def decoy(t):
    """Another valid input of the same shape, dtype and distribution: the rows of `t` moved on by one (every value stays one the
    call may meet — lengths in range, timesteps in [0, S), indices inside their tables).  Must differ from `t`."""
    d = t.roll(1, 0).contiguous()
    assert d.shape == t.shape and d.dtype == t.dtype and not torch.equal(d, t), "the decoy must differ from the true input"
    return d


def flat(out):
    """The tensors of a result (tensor, number, numpy array, or lists / tuples / dicts of them; None is skipped), in a fixed order."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, np.ndarray):
        return [torch.from_numpy(np.ascontiguousarray(out))]
    if isinstance(out, (bool, int, float)):
        return [torch.tensor(out)]
    if isinstance(out, dict):
        return [t for k in sorted(out, key=str) for t in flat(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for v in out for t in flat(v)]
    raise TypeError(type(out))


def keep(out):
    """Clones of a result's tensors on the current stream."""
    return [t.clone() for t in flat(out)]


def baseline(call, true):
    """call(*true) on the default stream -> its tensors, cloned; the device is idle afterwards.  Inputs are cloned: a call may
    work in place."""
    out = keep(call(*[t.clone() for t in true]))
    torch.cuda.synchronize()
    return out


class Side:
    def __init__(self, outs, pending, null_idle, host_ms):
        self.outs, self.pending, self.null_idle, self.host_ms = outs, pending, null_idle, host_ms


def side_run(call, true, stream, delay, decoys=None, prime=True):
    """The late-input run (module docstring).  -> Side: the cloned outputs; whether `stream` was still held when the call returned;
    whether the null stream was idle then; the host time of the call.  prime: the call first runs on the decoys, on the default
    stream, so that the workspace holds the decoys' intermediate results and not the baseline's: a kernel in the middle of a call
    that runs early then reads those, not values that happen to be right."""
    decoys = [decoy(t) for t in true] if decoys is None else decoys
    if prime:
        call(*[d.clone() for d in decoys])
    bufs = [d.clone() for d in decoys]
    true = [t.clone() for t in true]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay()
        for b, t in zip(bufs, true):
            b.copy_(t)
        t0 = time.perf_counter()
        out = call(*bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        null_idle = torch.cuda.default_stream().query()
        outs = keep(out)
    stream.synchronize()
    return Side(outs, pending, null_idle, host_ms)


def differing(got, want, rows=None):
    """None, or what differs between two lists of tensors (rows: per-window frame counts — only rows below them are compared)."""
    if len(got) != len(want):
        return f"{len(got)} results against {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"result {i}: {tuple(g.shape)} {g.dtype} against {tuple(w.shape)} {w.dtype}"
        if rows is not None and g.dim() >= 2 and g.shape[0] == len(rows):
            bad = [b for b, n in enumerate(rows) if not torch.equal(g[b, :n], w[b, :n])]
            if bad:
                return f"result {i}: windows {bad} differ below their lengths"
        elif not torch.equal(g, w):
            ne = g != w
            return f"result {i}: {int(ne.sum())} of {g.numel()} values differ"
    return None


def check(name, mode, call, true, stream, delay, want=None, decoys=None, rows=None, warm=True, prime=True):
    """Hold `call` to the checks of its `mode` (ENQUEUES, SYNCHRONISES, or a reason why the wrapper reads back: then only the bits
    and the null stream are checked).  want: the baseline's tensors (None: taken here, on the default stream).  warm=False: a first
    call of a shape (kernel attributes, graph capture): not held to the asynchrony check, and not primed.  prime: see side_run.
    -> the side run's outputs."""
    if want is None:
        want = baseline(call, true)
    r = side_run(call, true, stream, delay, decoys, prime and warm)
    d = differing(r.outs, want, rows)
    assert d is None, f"{name}: under a side stream with late inputs: {d}"
    assert r.null_idle, f"{name}: the null stream had work when the call returned"
    if mode == ENQUEUES and warm:
        assert r.pending, f"{name}: the call waited for its stream (host time {r.host_ms:.2f} ms, delay {delay.ms:.1f} ms)"
        delay.checked[name] = max(delay.checked.get(name, 0.), r.host_ms)
    elif mode == SYNCHRONISES:
        assert not r.pending, f"{name}: documented to synchronise, but its stream was still busy when it returned"
    return r.outs
