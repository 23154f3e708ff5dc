"""Controls for the stream-ordering harness (tests/stream_order.py) on the GPU, in pure torch: fake
"engines" made of tensor copies on a second stream T, each breaking one ordering edge of a call
on S.  Every fake must be flagged, else the engine tests that use the harness show nothing on
the device they run on.

The device runs a few hardware queues and streams share them: a T that lands on S's queue is
serialised behind S's delay and hides the missing edge on that run.  So each fake is tried on
up to 4 fresh streams and must be flagged on at least one.  Everything here touches only live
torch tensors."""
import numpy as np
import pytest
import torch

from stream_order import FIRST_FACTOR, Delay, Input, Output, Sandwich, run_checked

pytestmark = pytest.mark.gpu

SIZE = 1 << 20
TRIES = 4


def _dev():
    return torch.device("cuda", 0)


def _case(S):
    rng = np.random.default_rng(5)
    real, d1, d2 = (rng.integers(0, 256, SIZE, dtype=np.uint8) for _ in range(3))
    inp = Input(real, d1, d2, _dev())
    out = Output(SIZE, real, _dev())          # the operation: out = in
    return Sandwich(S, [inp], [out], _dev()), inp, out


def _delay_for(sw, call):
    """The warm-up pass of run_checked: the first delay from the host issue time."""
    sw.run(call, 0.0)
    assert sw.findings() == []
    return max(FIRST_FACTOR * sw.issue_s, 0.02)


def test_correct_fake_passes_and_is_pending(gpu):
    """The copy on T, forked from S and joined back: the contract holds, S was pending."""
    S, T = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    sw, inp, out = _case(S)

    def call(sw):
        T.wait_stream(S)
        with torch.cuda.stream(T):
            out.buf.copy_(inp.buf)
        S.wait_stream(T)

    rec = run_checked(sw, call, "control: correct fake")
    assert rec["pending"]


def _flagged_on_some_stream(fake, want, after=None):
    """Run `fake(sw, inp, out, T)` as the call on up to TRIES fresh streams T; True once a
    pending run produced a finding of kind `want`."""
    seen = []
    for _ in range(TRIES):
        S, T = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        sw, inp, out = _case(S)

        def good(sw):
            out.buf.copy_(inp.buf)

        delay_s = _delay_for(sw, good)
        sw.run(lambda sw: fake(sw, inp, out, T), delay_s)
        pending = sw.marked
        kinds = sorted({k for k, _ in sw.findings()})
        seen.append((pending, kinds))
        if pending and want in kinds and (after is None or after(inp, out)):
            return True, seen
    return False, seen


def test_reader_that_does_not_wait_for_s(gpu):
    """T reads the input without waiting for S: it sees decoy 1."""
    def fake(sw, inp, out, T):
        tmp = torch.empty_like(inp.buf)
        with torch.cuda.stream(T):
            tmp.copy_(inp.buf)
        sw.S.wait_stream(T)
        out.buf.copy_(tmp)
        sw.keep = tmp

    ok, seen = _flagged_on_some_stream(
        fake, "snapshot", lambda inp, out: torch.equal(out.snap, inp.decoy))
    assert ok, seen


def test_writer_that_does_not_wait_for_s(gpu):
    """T writes the (right) result without waiting for S: sentinel A lands on top of it."""
    def fake(sw, inp, out, T):
        with torch.cuda.stream(T):
            out.buf.copy_(inp.real)
        sw.S.wait_stream(T)

    ok, seen = _flagged_on_some_stream(fake, "snapshot")
    assert ok, seen


def test_writer_that_s_does_not_wait_for(gpu):
    """The result is written on S, then once more on T behind a longer delay of T's own, and S
    is not joined with T: the second write lands on sentinel B."""
    late = Delay(_dev(), lane=1)

    def fake(sw, inp, out, T):
        out.buf.copy_(inp.buf)
        keep = inp.buf.clone()
        T.wait_stream(sw.S)
        late.enqueue(T, 2 * sw.gate.seconds + 0.05)
        with torch.cuda.stream(T):
            out.buf.copy_(keep)
        sw.keep = keep

    ok, seen = _flagged_on_some_stream(fake, "late-output")
    assert ok, seen


def test_reader_that_s_does_not_wait_for(gpu):
    """T is forked from S but reads the input behind a delay of its own, and S is not joined
    with T: it reads decoy 2 and its result lands late."""
    late = Delay(_dev(), lane=1)

    def fake(sw, inp, out, T):
        T.wait_stream(sw.S)
        late.enqueue(T, 2 * sw.gate.seconds + 0.05)
        with torch.cuda.stream(T):
            out.buf.copy_(inp.buf)

    ok, seen = _flagged_on_some_stream(
        fake, "late-output", lambda inp, out: torch.equal(out.buf, inp.decoy2))
    assert ok, seen
