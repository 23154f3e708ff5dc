"""Stream-ordering harness: a time-bounded delay on a stream and a "sandwich" around calls that
promise stream order.  No engine code: torch tensors, streams and events only.

An entry point that enqueues on a caller's stream S and returns promises that (1) it reads its
inputs only after what the caller queued on S before the call, (2) what the caller queues on S
after the call sees the finished outputs, and (3) the caller may rewrite the inputs on S right
after the call.  On an idle stream all three hold whatever the callee does, so the sandwich holds
S busy with a delay while the call is issued and brackets it with decoys and sentinels, all
queued on S:

  0  the inputs hold decoy 1 (they still do when the host issues the call)
  1  the delay, then event E               pending() = not E.query()
  2  real bytes -> inputs
  3  sentinel A -> outputs
  4  the call(s), on S
  5  clones of the outputs (the snapshots)
  6  decoy 2 -> inputs
  7  sentinel B -> outputs

then S.synchronize() alone.  The snapshots must equal the reference (an input read early sees
decoy 1; an output written before the callee's fork is overwritten by sentinel A; an output not
finished where the call sits in S shows sentinel A or partial bytes).  After a final device
synchronize every output must hold sentinel B and every input decoy 2 (a callee stream that S
was not joined with writes late; a late read shows as a late write of decoy-2 results).  A run
in which S was not pending when the call returned proves nothing and is never counted as a pass
(run_checked doubles the delay and, failing that, fails).

The delay is a chain of in-place adds over a large tensor, sized from a timing of the same chain
on the device; the host never holds a gate, so a callee that blocks the host on pending device
work (a slot wait, a full upload ring) waits for the delay to run out and no longer.  Decoys are
valid data of the inputs' own kind, so an ordering bug shows as wrong bytes and nothing else.

With CPU tensors (stream None) every step runs in program order and the delay is a no-op: that
checks the bookkeeping (tests/test_stream_order_model.py)."""
import contextlib
import math
import time

import torch

CAP_S = 2.0            # no single delay is longer
FIRST_FACTOR = 10      # first delay = this many times the warm-up pass's host issue time
RETRIES = 3            # doublings of the delay when the stream was not pending
SENTINEL_A, SENTINEL_B = 0xA5, 0x3C
PAD_ELEMS = 64 << 20   # int32 elements of the delay's tensor (256 MiB)

REPORT = []            # one dict per checked run: label, issue_ms, delay_ms, ops, pending


@contextlib.contextmanager
def on(stream):
    if stream is None:
        yield
    else:
        with torch.cuda.stream(stream):
            yield


class _Pending:
    def __init__(self, event, ops, seconds):
        self.event, self.ops, self.seconds = event, ops, seconds

    def pending(self):
        """True while the delay (and so everything queued behind it) has not run."""
        return True if self.event is None else not self.event.query()


class Delay:
    """In-place adds over a 256 MiB tensor; the time of one add is measured once per device and
    lane (a lane is a tensor of its own, for a second delay running beside the first)."""
    _cal = {}

    def __init__(self, device, lane=0):
        self.device = torch.device(device)
        self.pad = self.per_op = None
        if self.device.type == "cpu":
            return
        key = (self.device.index, lane)
        if key not in Delay._cal:
            pad = torch.zeros(PAD_ELEMS, dtype=torch.int32, device=self.device)
            st = torch.cuda.Stream(self.device)
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            with torch.cuda.stream(st):
                for _ in range(10):
                    pad.add_(1)
                e0.record(st)
                for _ in range(50):
                    pad.add_(1)
                e1.record(st)
            e1.synchronize()
            Delay._cal[key] = (pad, e0.elapsed_time(e1) / 50 / 1000.0)
        self.pad, self.per_op = Delay._cal[key]

    def ops_for(self, seconds):
        if self.per_op is None or seconds <= 0:
            return 0
        return max(1, math.ceil(min(seconds, CAP_S) / self.per_op))

    def enqueue(self, stream, seconds):
        """Queue about `seconds` (at most CAP_S) of work on `stream`, then an event."""
        ops = self.ops_for(seconds)
        if self.pad is None:
            return _Pending(None, 0, 0.0)
        with torch.cuda.stream(stream):
            for _ in range(ops):
                self.pad.add_(1)
            ev = torch.cuda.Event()
            ev.record(stream)
        return _Pending(ev, ops, ops * self.per_op)


def _dev_tensor(a, device):
    # (torch.tensor copies: the shared references are read-only numpy arrays)
    t = a if isinstance(a, torch.Tensor) else torch.tensor(a)
    return t.reshape(-1).to(device).contiguous()


class Input:
    """A device input: its real bytes and two decoys of the same size.  `stream`: the stream its
    steps are queued on (default: the sandwich's S)."""

    def __init__(self, real, decoy, decoy2, device, stream=None, name="input"):
        self.real, self.decoy, self.decoy2 = (_dev_tensor(x, device) for x in (real, decoy, decoy2))
        assert self.real.shape == self.decoy.shape == self.decoy2.shape, name
        assert self.real.dtype == self.decoy.dtype == self.decoy2.dtype, name
        assert not torch.equal(self.real, self.decoy) and not torch.equal(self.real, self.decoy2), \
            name + ": a decoy equal to the real bytes shows nothing"
        self.buf = self.decoy.clone()
        self.stream, self.name = stream, name

    @property
    def ptr(self):
        return self.buf.data_ptr()


class Output:
    """An output buffer of `size` bytes.  `ref`: the bytes the snapshot must hold at `select`
    (an index tensor; None = the whole buffer) -- where the callee is to leave bytes alone inside
    `select`, the reference holds SENTINEL_A there.  `stream`: where its fills are queued
    (default S); `snap_stream`: where its snapshot is taken (default `stream`)."""

    def __init__(self, size, ref, device, select=None, stream=None, snap_stream=None,
                 name="output"):
        self.buf = torch.full((size,), SENTINEL_A, dtype=torch.uint8, device=device)
        self.ref = _dev_tensor(ref, device)
        self.select = None if select is None else _dev_tensor(select, device)
        assert self.ref.numel() == (size if select is None else self.select.numel()), name
        self.stream, self.snap_stream, self.name = stream, snap_stream, name
        self.snap = None

    @property
    def ptr(self):
        return self.buf.data_ptr()


class Sandwich:
    """Steps 0-7 around `call(sandwich)` on stream S (None: CPU tensors, program order).  `join`:
    streams S is made to wait for between the snapshots and step 6 (a stream the callee released
    early, on which a snapshot was taken)."""

    def __init__(self, stream, inputs, outputs, device, join=(), lane=0):
        self.S, self.inputs, self.outputs = stream, list(inputs), list(outputs)
        self.device, self.join = torch.device(device), list(join)
        self.delay = Delay(device, lane)
        self.gate = None
        self.marked = None
        self.issue_s = 0.0

    def _st(self, item_stream):
        return self.S if item_stream is None else item_stream

    def pending(self):
        return self.gate.pending()

    def mark(self):
        """Called by `call` at its sensitivity point (default: when it returns)."""
        if self.marked is None:
            self.marked = self.pending()
        return self.marked

    def front(self, delay_s):
        for i in self.inputs:                                   # 0
            with on(self._st(i.stream)):
                i.buf.copy_(i.decoy)
        self.marked = None
        self.gate = self.delay.enqueue(self.S, delay_s)         # 1
        self._t0 = time.perf_counter()
        for i in self.inputs:                                   # 2
            with on(self._st(i.stream)):
                i.buf.copy_(i.real)
        for o in self.outputs:                                  # 3
            with on(self._st(o.stream)):
                o.buf.fill_(SENTINEL_A)

    def issue(self, call):
        with on(self.S):
            out = call(self)                                    # 4
        self.mark()
        self.issue_s = time.perf_counter() - self._t0
        return out

    def back(self):
        for o in self.outputs:                                  # 5
            with on(self._st(o.snap_stream if o.snap_stream is not None else o.stream)):
                o.snap = o.buf.clone()
        if self.S is not None:
            for j in self.join:
                self.S.wait_stream(j)
        for i in self.inputs:                                   # 6
            with on(self._st(i.stream)):
                i.buf.copy_(i.decoy2)
        for o in self.outputs:                                  # 7
            with on(self._st(o.stream)):
                o.buf.fill_(SENTINEL_B)

    def findings(self):
        """Stream synchronizes, the snapshot comparison, a device synchronize, the late checks.
        Returns a list of (kind, text): kind in "snapshot", "late-output", "late-input"."""
        found = []
        if self.S is not None:
            self.S.synchronize()
            for x in self.inputs + self.outputs:
                for st in (x.stream, getattr(x, "snap_stream", None)):
                    if st is not None:
                        st.synchronize()
        for o in self.outputs:
            got = o.snap if o.select is None else o.snap[o.select]
            if not torch.equal(got, o.ref):
                bad = torch.nonzero(got != o.ref).reshape(-1)
                a = int((got[bad] == SENTINEL_A).sum())
                found.append(("snapshot", f"{o.name}: snapshot differs from the reference in "
                              f"{bad.numel()} of {got.numel()} bytes (first at {int(bad[0])}; "
                              f"{a} of them hold sentinel A)"))
        if self.S is not None:
            torch.cuda.synchronize(self.device)
        for o in self.outputs:
            if not bool((o.buf == SENTINEL_B).all()):
                found.append(("late-output", f"{o.name}: written after sentinel B "
                              f"({int((o.buf != SENTINEL_B).sum())} bytes)"))
        for i in self.inputs:
            if not torch.equal(i.buf, i.decoy2):
                found.append(("late-input", f"{i.name}: not the second decoy at the end"))
        return found

    def run(self, call, delay_s):
        self.front(delay_s)
        out = self.issue(call)
        self.back()
        return out


def run_checked(sw, call, label, check=None):
    """The warm-up pass on an idle stream (its bytes are checked too), then the sandwich behind a
    delay of FIRST_FACTOR times the warm-up's host issue time, doubled up to RETRIES times (within
    CAP_S) while the stream was not pending at the sensitivity point.  `check(result)`: asserts on
    what `call` returned.  Fails on any finding, and when no run was pending."""
    out = sw.run(call, 0.0)
    found = sw.findings()
    assert not found, f"{label} (idle stream): {found}"
    if check:
        check(out)
    issue_s = sw.issue_s
    delay_s = min(FIRST_FACTOR * issue_s, CAP_S)
    for attempt in range(RETRIES + 1):
        out = sw.run(call, delay_s)
        was_pending = sw.marked
        found = sw.findings()
        rec = {"label": label, "issue_ms": round(issue_s * 1e3, 3),
               "delay_ms": round(sw.gate.seconds * 1e3, 3), "ops": sw.gate.ops,
               "attempt": attempt, "pending": bool(was_pending)}
        REPORT.append(rec)
        print("stream-order:", rec)
        assert not found, f"{label} (pending={was_pending}, delay {rec['delay_ms']} ms): {found}"
        if check:
            check(out)
        if was_pending:
            return rec
        if delay_s >= CAP_S:
            break
        delay_s = min(2 * delay_s, CAP_S)
    raise AssertionError(f"{label}: the stream was never pending at the sensitivity point "
                         f"(last delay {delay_s * 1e3:.1f} ms): the run proves nothing")
