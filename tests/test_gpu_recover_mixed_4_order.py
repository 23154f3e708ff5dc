"""Stream order of rs2_sliver_checker_recover_device_async (tests/stream_order.py, used as
tests/test_gpu_verify_mixed_4_order.py uses it): the call is issued behind a delay on the caller's
stream -- a torch stream, and torch's default stream passed as RS2_STREAM_LEGACY -- between decoys
and sentinels queued on the same stream.  Input: the received symbols; its decoys are other valid
symbols in the same layout, so bytes read too early or too late show as another sliver.  Outputs:
slivers, roots and verdicts.  The HOST arrays are overwritten with other valid values as soon as
the call returns.

The checker's own stream (stream NULL): three calls back to back without a synchronize between
them, and -- because a mixed verification and a mixed recovery share the checker's scratch and
tables -- a verification interleaved between two recoveries.  Two streams, one checker: call A
sits behind a delay on stream 1, call B on the idle stream 2 must order itself after A."""
import ctypes

import numpy as np
import pytest
import torch

import recover_mixed as R
import verify_mixed as M
from stream_order import Delay, Input, Output, Sandwich, run_checked
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 100
SIZES = [6, 66, 130, 258]


def _case(shift):
    """The same layout and patterns with other slivers: seeds shifted."""
    return [(a, s, p, (seed + shift) % M.POOL) for a, s, p, seed in R.family_case(N, SIZES)[:24]]


def _rewrite(arr, values):
    for i, x in enumerate(values):
        arr[i] = x


@pytest.mark.parametrize("kind", ["stream", "legacy"])
def test_caller_stream(gpu, kind):
    dev = R.dev()
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    cases = [_case(k) for k in range(3)]
    items = cases[0]
    m = len(items)
    s_off, s_size, o_off, o_size = R.layout(N, items, gap=0)
    bufs = [R.payload(N, c, s_off, s_size) for c in cases]
    want = R.expected_roots(N, items)
    expected = bytearray(want)
    expected[32:64] = want[0:32]                  # a mismatch among the matches
    verdicts = np.array([R.MATCH] * m, dtype=np.int32)
    verdicts[1] = R.MISMATCH
    slivers = np.frombuffer(b"".join(R.want_sliver(N, it) for it in items), dtype=np.uint8)
    assert slivers.size == o_size
    sym = Input(*bufs, dev, name="d_symbols")
    out = Output(o_size, slivers, dev, name="d_slivers")
    roots = Output(m * 32, np.frombuffer(want, dtype=np.uint8), dev, name="d_roots")
    verdict = Output(m * 4, verdicts.view(np.uint8), dev, name="d_verdict")
    checker = gpu.SliverChecker(N)
    flat = [q for _, _, p, _ in items for q in p]
    a_ax, a_sz = (ctypes.c_uint8 * m)(), (ctypes.c_uint16 * m)()
    a_cnt, a_idx = (ctypes.c_uint32 * m)(), (ctypes.c_uint16 * len(flat))()
    a_so, a_oo = (ctypes.c_uint64 * m)(), (ctypes.c_uint64 * m)()
    a_exp = (ctypes.c_uint8 * (m * 32))()

    def call(sw):
        _rewrite(a_ax, [R.AXES.index(a) for a, _, _, _ in items])
        _rewrite(a_sz, [s for _, s, _, _ in items])
        _rewrite(a_cnt, [len(p) for _, _, p, _ in items])
        _rewrite(a_idx, flat)
        _rewrite(a_so, s_off)
        _rewrite(a_oo, o_off)
        ctypes.memmove(a_exp, bytes(expected), m * 32)
        rc = _lib.lib().rs2_sliver_checker_recover_device_async(
            checker.handle, m, a_ax, a_sz, a_cnt, a_idx, sym.ptr, a_so, a_exp, out.ptr, a_oo,
            roots.ptr, verdict.ptr, None, ctypes.c_void_p(S.cuda_stream or 1))
        sw.mark()
        # other valid values: the sizes rotated, the indices and offsets reversed
        _rewrite(a_sz, [items[(i + 1) % m][1] for i in range(m)])
        _rewrite(a_idx, flat[::-1])
        _rewrite(a_so, s_off[::-1])
        _rewrite(a_oo, o_off[::-1])
        ctypes.memmove(a_exp, bytes(want[::-1]), m * 32)
        return rc

    def check(rc):
        assert rc == 0, (rc, _lib.last_error())

    rec = run_checked(Sandwich(S, [sym], [out, roots, verdict], dev), call,
                      f"sliver_checker_recover {kind}", check)
    assert rec["pending"]


def _buffers(case):
    m = len(case)
    s_off, s_size, o_off, o_size = R.layout(N, case)
    return dict(sym=torch.tensor(R.payload(N, case, s_off, s_size), dtype=torch.uint8, device=R.dev()),
                s_off=s_off, o_off=o_off,
                out=torch.full((o_size,), R.FILL, dtype=torch.uint8, device=R.dev()),
                roots=torch.full((m * 32,), R.FILL, dtype=torch.uint8, device=R.dev()),
                verdict=torch.full((m,), -1, dtype=torch.int32, device=R.dev()))


def _issue(checker, case, b, stream=None):
    rc = checker.recover_async([a for a, _, _, _ in case], [s for _, s, _, _ in case],
                               [p for _, _, p, _ in case], b["sym"].data_ptr(), b["s_off"],
                               b["out"].data_ptr(), b["o_off"], R.expected_roots(N, case),
                               b["roots"].data_ptr(), b["verdict"].data_ptr(), stream)
    assert rc == 0, (rc, _lib.last_error())


def _verify(case, b, what):
    R.check_slivers(N, case, b["out"].cpu().numpy(), b["o_off"], what=what)
    R.check_roots(N, case, b["roots"].cpu().numpy().tobytes(), what=what)
    assert b["verdict"].cpu().tolist() == [R.MATCH] * len(case), what


def test_own_stream_back_to_back_with_a_verification_between(gpu):
    checker = gpu.SliverChecker(N)
    big = R.family_case(N, R.SIZES, repeat=2)
    cases = [big, _case(1), _case(2)]
    bufs = [_buffers(c) for c in cases]
    v_case = M.groups_case(N, [6, 66, 130], 2, "interleaved")
    v_off, v_size = M.layout(N, v_case)
    v_in = torch.tensor(M.payload(N, v_case, v_off, v_size), dtype=torch.uint8, device=R.dev())
    v_roots = torch.full((len(v_case) * 32,), R.FILL, dtype=torch.uint8, device=R.dev())
    for c in cases:
        R.expected_roots(N, c)                   # references first: no host work between calls
    M.expected_roots(N, v_case)
    torch.cuda.synchronize()
    _issue(checker, cases[0], bufs[0])
    _issue(checker, cases[1], bufs[1])
    rc = checker.verify_async([a for a, _, _ in v_case], [s for _, s, _ in v_case],
                              v_in.data_ptr(), v_off, None, v_roots.data_ptr())
    assert rc == 0, (rc, _lib.last_error())
    _issue(checker, cases[2], bufs[2])
    torch.cuda.synchronize()
    for i, (c, b) in enumerate(zip(cases, bufs)):
        _verify(c, b, f"call {i}")
    M.check_roots(N, v_case, v_roots.cpu().numpy().tobytes(), what="the verification between")


def test_two_streams_one_checker(gpu):
    dev = R.dev()
    checker = gpu.SliverChecker(N)
    cases = [_case(1), _case(3)]
    bufs = [_buffers(c) for c in cases]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for k in (0, 1):                             # warm-up: codes, buffers
        _issue(checker, cases[k], bufs[k], streams[k].cuda_stream)
    torch.cuda.synchronize()
    for b in bufs:
        b["out"].fill_(R.FILL), b["roots"].fill_(R.FILL), b["verdict"].fill_(-1)
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
