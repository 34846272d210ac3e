"""The rig of tests/test_gpu_caller_stream.py: a context bound to a stream the CALLER owns and keeps busy.

A library call is made in one of two modes through the same object, so a test writes its sequence once:

  idle   the inputs are written and the stream is drained before the call; nothing is asserted about time.  The host
         time of every enqueue-only call is measured here (warmed: the second idle run of a sequence);
  held   a bounded spin (torch.cuda._sleep) is enqueued on the stream, then an event (the marker), then the torch kernels
         that write the real inputs over the decoys the buffers were prefilled with -- and the library call follows at
         once.  An enqueue-only call must return while the marker is still pending (`enqueue`); a synchronising one must
         be entered while it is pending (`blocking`).  Both are asserted: a hold that ran out proves nothing.

The hold is max(HOLD_MIN_MS, HOLD_FACTOR x the slowest enqueue-only call seen so far); a call slower than
HOLD_MAX_MS / HOLD_FACTOR fails its validity assertion instead of lengthening the spin without bound."""
import time

import numpy as np
import torch

HOLD_MIN_MS = 20.0
HOLD_FACTOR = 10.0
HOLD_MAX_MS = 500.0
POISON = 0x0BAD0BAD0BAD0BAD                  # what an output buffer holds before a run and after it was consumed (int64)


def dev(arr):
    """A host array as a device tensor of the same bytes (uint64 words travel as int64, uint32 as int32)."""
    a = np.ascontiguousarray(arr)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def host(t, dtype=np.uint64):
    """A device tensor's bytes as a host array of `dtype`."""
    return t.cpu().numpy().view(dtype)


def norm(x):
    """A result (arrays, device tensors, tuples of them, flags, bytes) as nested tuples of bytes and plain values."""
    if isinstance(x, torch.Tensor):
        return x.cpu().numpy().tobytes()
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).tobytes()
    if isinstance(x, (list, tuple)):
        return tuple(norm(v) for v in x)
    if isinstance(x, (np.bool_, np.integer)):
        return x.item()
    return x


class _Mode:
    def __init__(self, rig, held, warm=True):
        self.rig, self.held, self.warm, self.marker = rig, held, warm, None
        self.entered = []          # (name, marker pending on entry), held mode
        self.returned = []         # (name, marker pending on return), held mode, enqueue-only calls

    # -- the caller's side ---------------------------------------------------------------------------------------
    def begin(self, writes=()):
        """Starts a hold (held mode) and enqueues the caller's kernels that write its inputs: (buffer, value) pairs."""
        rig = self.rig
        with torch.cuda.stream(rig.stream):
            if self.held:
                torch.cuda._sleep(rig.hold_cycles())
                self.marker = torch.cuda.Event()
                self.marker.record()
            for buf, val in writes:
                buf.copy_(val)
        if not self.held:
            rig.stream.synchronize()

    def consume(self, out):
        """The caller's next kernel on the stream reads `out`; the buffer is overwritten afterwards."""
        with torch.cuda.stream(self.rig.stream):
            c = out.clone()
            out.fill_(POISON if out.dtype == torch.int64 else 0x5A)
        return c

    # -- the library's side --------------------------------------------------------------------------------------
    def enqueue(self, name, fn, *a, may_wait=False, **kw):
        """An enqueue-only entry: returns while the hold lasts (may_wait: only entered while it lasts)."""
        pending = self.held and not self.marker.query()
        t0 = time.perf_counter()
        r = fn(*a, **kw)
        dt = time.perf_counter() - t0
        if self.held:
            self.entered.append((name, pending))
            if not may_wait:
                self.returned.append((name, not self.marker.query(), dt))
        elif self.warm and not may_wait:
            self.rig.note_enqueue(name, dt)
        return r

    def blocking(self, name, fn, *a, **kw):
        """An entry that synchronises: entered while the hold lasts."""
        if self.held:
            self.entered.append((name, not self.marker.query()))
        return fn(*a, **kw)

    def finish(self):
        self.rig.stream.synchronize()
        for name, pending in self.entered:
            assert pending, "%s: the hold (%.1f ms) ran out before the call was made: the run proves nothing" % (name, self.rig.hold_ms())
        for name, pending, dt in self.returned:
            assert pending, ("%s is documented as enqueue-only but returned after the work the caller had put on the stream "
                             "was done (%.2f ms in the call, hold %.1f ms): it synchronised" % (name, dt * 1e3, self.rig.hold_ms()))


class Rig:
    """One context on one caller-owned stream.  stream = None: torch's default stream, handle 0."""

    def __init__(self, ctx, stream=None):
        self.ctx = ctx
        self.stream = torch.cuda.default_stream() if stream is None else stream
        ctx.set_stream(self.stream.cuda_stream)
        self.cycles_per_ms = None
        self.slowest = ("", 0.0)          # the slowest warmed enqueue-only call: (name, seconds)
        self.held_calls = 0

    def calibrate(self):
        """Spin cycles per millisecond, from one timed spin on the idle stream."""
        cycles = 20_000_000
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(1000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "torch.cuda._sleep(%d) took %.3f ms: no hold can be built from it" % (cycles, ms)
        self.cycles_per_ms = cycles / ms
        return self.cycles_per_ms

    def share_calibration(self, other):
        self.cycles_per_ms = other.cycles_per_ms

    def note_enqueue(self, name, seconds):
        if seconds > self.slowest[1]:
            self.slowest = (name, seconds)

    def hold_ms(self):
        want = max(HOLD_MIN_MS, HOLD_FACTOR * self.slowest[1] * 1e3)
        assert want <= HOLD_MAX_MS, ("%s took %.1f ms of host time on an idle stream: no bounded hold is ten times that"
                                     % (self.slowest[0], self.slowest[1] * 1e3))
        return want

    def hold_cycles(self):
        if self.cycles_per_ms is None:
            self.calibrate()
        self.held_calls += 1
        return int(self.hold_ms() * self.cycles_per_ms)

    def fill(self, pairs):
        """Synchronously: every buffer holds its value before anything else happens."""
        with torch.cuda.stream(self.stream):
            for buf, val in pairs:
                if isinstance(val, torch.Tensor):
                    buf.copy_(val)
                else:
                    buf.fill_(val)
        self.stream.synchronize()

    def three_ways(self, body, bufs, decoys, reals, outs=()):
        """body(mode, data) makes the caller's writes through mode.begin and the library calls through mode.enqueue /
        mode.blocking, and returns the results.  Run on the idle stream over the decoys (first run: everything lazy is
        allocated here), on the idle stream over the real inputs, and on the held stream with the real inputs written
        behind the hold over the decoys.  -> (decoy, idle, held) results in norm() form."""
        res = []
        for held, data, pre in ((False, decoys, decoys), (False, reals, decoys), (True, reals, decoys)):
            self.fill(list(zip(bufs, pre)) + [(o, POISON if o.dtype == torch.int64 else 0x5A) for o in outs])
            mode = _Mode(self, held, warm=bool(res))          # the first run is the warm-up: its host times do not count
            r = body(mode, data)
            mode.finish()
            res.append(norm(r))
        return tuple(res)


def compare(name, results, want, decoy_differs=True):
    """held == idle == oracle, exactly; says so when the held run computed the decoy's answer."""
    decoy, idle, held = results
    want = norm(want)
    if decoy_differs:
        assert decoy != want, "%s: the decoy's answer equals the real one: a stale read would go unseen" % name
    assert idle == want, "%s: wrong on the idle stream" % name
    if held != want:
        what = ("it is the DECOY's answer: the call read the caller's buffer before the caller's kernel on the stream had written it"
                if held == decoy else "it is neither the real answer nor the decoy's")
        raise AssertionError("%s: wrong on the held stream; %s" % (name, what))
