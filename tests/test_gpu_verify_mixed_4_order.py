"""Stream order of rs2_sliver_checker_verify_device_async (tests/stream_order.py, used as
tests/test_gpu_symbols_multi_4_order.py uses it): the call is issued behind a delay on the caller's
stream -- a torch stream, and torch's default stream passed as RS2_STREAM_LEGACY -- between decoys
and sentinels queued on the same stream.  Input: the slivers' buffer; its decoys are other valid
slivers in the same layout, so bytes read too early or too late show as another sliver's root.
Outputs: roots and verdicts.  The HOST arrays (axes, sizes, offsets, expected roots) are
overwritten with other valid values as soon as the call returns.

The checker's own stream (stream NULL) has no handle a delay could be queued on; there, three
calls are issued back to back without a synchronize between them -- a large one to keep the stream
busy, then two with different slivers into different outputs -- so the second reuses the first's
scratch and tables while they may still be read: stream order alone must keep both right.

Two streams, one checker: call A sits behind a delay on stream 1, call B is issued on the idle
stream 2.  B reuses A's scratch, so it must order itself after A: while the delay is pending B may
not have finished, and both results are right at the end."""
import ctypes

import numpy as np
import pytest
import torch

import verify_mixed as M
from stream_order import Delay, Input, Output, Sandwich, run_checked
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 100
SIZES = [2, 6, 66, 130]      # s = 2: the per-size path runs inside the same call


def _case(shift):
    """The same layout with other slivers: seeds shifted."""
    return [(a, s, (seed + shift) % M.POOL) for a, s, seed in M.groups_case(N, SIZES, 2, "interleaved")]


def _rewrite(arr, values):
    for i, x in enumerate(values):
        arr[i] = x


@pytest.mark.parametrize("kind", ["stream", "legacy"])
def test_caller_stream(gpu, kind):
    dev = M.dev()
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    cases = [_case(k) for k in range(3)]
    items = cases[0]
    m = len(items)
    off, size = M.layout(N, items)
    bufs = [M.payload(N, c, off, size) for c in cases]
    want = M.expected_roots(N, items)
    # one sliver's expected root is another sliver's: a mismatch among the matches
    expected = bytearray(want)
    expected[32:64] = want[0:32]
    verdicts = np.array([M.MATCH] * m, dtype=np.int32)
    verdicts[1] = M.MISMATCH
    slv = Input(*bufs, dev, name="d_slivers")
    roots = Output(m * 32, np.frombuffer(want, dtype=np.uint8), dev, name="d_roots")
    verdict = Output(m * 4, verdicts.view(np.uint8), dev, name="d_verdict")
    checker = gpu.SliverChecker(N)
    a_ax, a_sz = (ctypes.c_uint8 * m)(), (ctypes.c_uint16 * m)()
    a_off, a_exp = (ctypes.c_uint64 * m)(), (ctypes.c_uint8 * (m * 32))()

    def call(sw):
        _rewrite(a_ax, [M.AXES.index(a) for a, _, _ in items])
        _rewrite(a_sz, [s for _, s, _ in items])
        _rewrite(a_off, off)
        ctypes.memmove(a_exp, bytes(expected), m * 32)
        rc = _lib.lib().rs2_sliver_checker_verify_device_async(
            checker.handle, m, a_ax, a_sz, slv.ptr, a_off, a_exp, roots.ptr, verdict.ptr, None,
            ctypes.c_void_p(S.cuda_stream or 1))
        sw.mark()
        # other valid values: the two axes swapped, the sizes rotated, the offsets reversed
        _rewrite(a_ax, [1 - M.AXES.index(a) for a, _, _ in items])
        _rewrite(a_sz, [items[(i + 1) % m][1] for i in range(m)])
        _rewrite(a_off, off[::-1])
        ctypes.memmove(a_exp, bytes(want[::-1]), m * 32)
        return rc

    def check(rc):
        assert rc == 0, (rc, _lib.last_error())

    rec = run_checked(Sandwich(S, [slv], [roots, verdict], dev), call,
                      f"sliver_checker_verify {kind}", check)
    assert rec["pending"]


def _buffers(case):
    off, size = M.layout(N, case)
    m = len(case)
    return (torch.tensor(M.payload(N, case, off, size), dtype=torch.uint8, device=M.dev()), off,
            torch.full((m * 32,), M.FILL, dtype=torch.uint8, device=M.dev()),
            torch.full((m,), -1, dtype=torch.int32, device=M.dev()))


def _issue(checker, case, bufs, stream=None):
    d_in, off, d_roots, d_verdict = bufs
    rc = checker.verify_async([a for a, _, _ in case], [s for _, s, _ in case], d_in.data_ptr(),
                              off, M.expected_roots(N, case), d_roots.data_ptr(),
                              d_verdict.data_ptr(), stream)
    assert rc == 0, (rc, _lib.last_error())


def _verify(case, bufs, what):
    _, _, d_roots, d_verdict = bufs
    M.check_roots(N, case, d_roots.cpu().numpy().tobytes(), what=what)
    assert d_verdict.cpu().tolist() == [M.MATCH] * len(case), what


def test_own_stream_back_to_back(gpu):
    checker = gpu.SliverChecker(N)
    big = M.groups_case(N, [s for s in M.SIZES if s >= 4], 5, "sorted", big=("primary", 258, 65))
    cases = [big, _case(1), _case(2)]
    bufs = [_buffers(c) for c in cases]
    for c in cases:
        M.expected_roots(N, c)                   # references first: no host work between calls
    torch.cuda.synchronize()
    for c, b in zip(cases, bufs):
        _issue(checker, c, b)
    torch.cuda.synchronize()
    for i, (c, b) in enumerate(zip(cases, bufs)):
        _verify(c, b, f"call {i}")


def test_two_streams_one_checker(gpu):
    dev = M.dev()
    checker = gpu.SliverChecker(N)
    cases = [_case(1), _case(3)]
    bufs = [_buffers(c) for c in cases]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for k in (0, 1):                             # warm-up: codes, buffers
        _issue(checker, cases[k], bufs[k], streams[k].cuda_stream)
    torch.cuda.synchronize()
    for b in bufs:
        b[2].fill_(M.FILL), b[3].fill_(-1)
    torch.cuda.synchronize()
    delay = Delay(dev)
    seconds, ordered = 0.25, None
    for _ in range(3):
        gate = delay.enqueue(streams[0], seconds)
        _issue(checker, cases[0], bufs[0], streams[0].cuda_stream)
        _issue(checker, cases[1], bufs[1], streams[1].cuda_stream)
        done_b = torch.cuda.Event()
        done_b.record(streams[1])
        finished = done_b.query()
        if gate.pending():               # A cannot have run yet: B may not be through either
            ordered = not finished
            break
        torch.cuda.synchronize()
        seconds *= 2
    torch.cuda.synchronize()
    assert ordered is not None, "stream 1 was never pending when both calls had been issued"
    assert ordered, "call B finished on stream 2 while call A, whose scratch it reuses, had not run"
    for k in (0, 1):
        _verify(cases[k], bufs[k], f"stream {k + 1}")
