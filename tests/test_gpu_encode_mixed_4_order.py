"""Stream order of rs2_blob_encoder_encode_device_async (tests/stream_order.py, used as
tests/test_gpu_verify_mixed_4_order.py uses it): the call is issued behind a delay on the caller's
stream -- a torch stream, and torch's default stream passed as RS2_STREAM_LEGACY -- between decoys
and sentinels queued on the same stream.  Input: the blobs' buffer; its decoys are other blobs in
the same layout, so bytes read too early or too late show as another blob's slivers and id.
Outputs: slivers, pair hashes and ids.  The HOST arrays (lengths, offsets) are overwritten with
other valid values as soon as the call returns.  Every blob here is eligible for the group
launches: only that path promises never to wait for the device.

The encoder's own stream (stream NULL) has no handle a delay could be queued on; there, three calls
are issued back to back without a synchronize between them -- a large one to keep the stream busy,
then two with different blobs into different outputs -- so the second reuses the first's scratch
and tables while they may still be read: stream order alone must keep both right.

Two streams, one encoder: call A sits behind a delay on stream 1, call B is issued on the idle
stream 2.  B reuses A's scratch, so it must order itself after A: while the delay is pending B may
not have finished, and both results are right at the end."""
import ctypes

import numpy as np
import pytest
import torch

import encode_mixed as M
from stream_order import SENTINEL_A, Delay, Input, Output, Sandwich, run_checked
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 100
SIZES = [4, 6, 66, 130]


def _case(shift):
    """The same layout with other blobs: seeds shifted."""
    return [(x, seed + shift) for x, seed in M.case(N, SIZES, 1, "interleaved")]


def _rewrite(arr, values):
    for i, x in enumerate(values):
        arr[i] = x


def _expected(lay, what):
    """A whole output buffer as the snapshot must show it: the references at their offsets,
    sentinel A wherever the call writes nothing."""
    offs, lens, size = {"primary": (lay.prim_off, lay.prim_len, lay.prim_bytes),
                        "secondary": (lay.sec_off, lay.sec_len, lay.sec_bytes)}[what]
    buf = torch.full((size,), SENTINEL_A, dtype=torch.uint8, device=M.dev())
    for (x, seed), o, ln in zip(lay.items, offs, lens):
        buf[o:o + ln] = getattr(M.reference(N, x, seed), what)
    return buf


@pytest.mark.parametrize("kind", ["stream", "legacy"])
def test_caller_stream(gpu, kind):
    dev = M.dev()
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    cases = [_case(k) for k in range(3)]
    items = cases[0]
    m = len(items)
    lays = [M.Layout(N, c) for c in cases]
    lay = lays[0]
    blobs = Input(*[lz.blobs() for lz in lays], dev, name="d_blobs")
    refs = [M.reference(N, x, seed) for x, seed in items]
    outs = [Output(lay.prim_bytes, _expected(lay, "primary"), dev, name="d_primary"),
            Output(lay.sec_bytes, _expected(lay, "secondary"), dev, name="d_secondary"),
            Output(m * N * 64, torch.cat([r.hashes for r in refs]), dev, name="d_hashes"),
            Output(m * 32, torch.cat([r.blob_id for r in refs]), dev, name="d_blob_ids")]
    enc = gpu.BlobEncoder(N)
    a_len, a_boff = (ctypes.c_uint64 * m)(), (ctypes.c_uint64 * m)()
    a_poff, a_soff = (ctypes.c_uint64 * m)(), (ctypes.c_uint64 * m)()
    lens = [x for x, _ in items]

    def call(sw):
        _rewrite(a_len, lens)
        _rewrite(a_boff, lay.blob_off)
        _rewrite(a_poff, lay.prim_off)
        _rewrite(a_soff, lay.sec_off)
        rc = _lib.lib().rs2_blob_encoder_encode_device_async(
            enc.handle, m, a_len, blobs.ptr, a_boff, outs[0].ptr, a_poff, outs[1].ptr, a_soff,
            outs[2].ptr, outs[3].ptr, None, ctypes.c_void_p(S.cuda_stream or 1))
        sw.mark()
        # other valid values: the lengths rotated, the offsets reversed
        _rewrite(a_len, lens[1:] + lens[:1])
        _rewrite(a_boff, lay.blob_off[::-1])
        _rewrite(a_poff, lay.prim_off[::-1])
        _rewrite(a_soff, lay.sec_off[::-1])
        return rc

    def check(rc):
        assert rc == 0, (rc, _lib.last_error())

    rec = run_checked(Sandwich(S, [blobs], outs, dev), call, f"blob_encoder_encode {kind}", check)
    assert rec["pending"]


def _buffers(case):
    lay = M.Layout(N, case)
    m = len(case)
    full = lambda k: torch.full((k,), M.FILL, dtype=torch.uint8, device=M.dev())  # noqa: E731
    return (lay, torch.tensor(lay.blobs(), device=M.dev()), full(lay.prim_bytes),
            full(lay.sec_bytes), full(m * N * 64), full(m * 32))


def _issue(enc, case, bufs, stream=None):
    lay, d_in, prim, sec, hashes, ids = bufs
    rc = enc.encode_async([x for x, _ in case], d_in.data_ptr(), lay.blob_off, prim.data_ptr(),
                          lay.prim_off, sec.data_ptr(), lay.sec_off, hashes.data_ptr(),
                          ids.data_ptr(), stream)
    assert rc == 0, (rc, _lib.last_error())


def _verify(bufs, what):
    lay, _, prim, sec, hashes, ids = bufs
    M.check(N, M.Out(0, lay, prim, sec, hashes, ids), what)


def _reset(bufs):
    for t in bufs[2:]:
        t.fill_(M.FILL)


def test_own_stream_back_to_back(gpu):
    enc = gpu.BlobEncoder(N)
    big = [(x, seed) for x, seed in M.case(N, [s for s in M.SIZES if s >= 4], 5, "sorted")]
    cases = [big, _case(1), _case(0)]
    bufs = [_buffers(c) for c in cases]
    for c in cases:
        for x, seed in c:
            M.reference(N, x, seed)              # references first: no host work between calls
    torch.cuda.synchronize()
    for c, b in zip(cases, bufs):
        _issue(enc, c, b)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        _verify(b, f"call {i}")


def test_two_streams_one_encoder(gpu):
    dev = M.dev()
    enc = gpu.BlobEncoder(N)
    cases = [_case(1), _case(0)]
    bufs = [_buffers(c) for c in cases]
    for c in cases:
        for x, seed in c:
            M.reference(N, x, seed)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for k in (0, 1):                             # warm-up: templates, buffers
        _issue(enc, cases[k], bufs[k], streams[k].cuda_stream)
    torch.cuda.synchronize()
    for b in bufs:
        _reset(b)
    torch.cuda.synchronize()
    delay = Delay(dev)
    seconds, ordered = 0.25, None
    for _ in range(3):
        gate = delay.enqueue(streams[0], seconds)
        _issue(enc, cases[0], bufs[0], streams[0].cuda_stream)
        _issue(enc, cases[1], bufs[1], streams[1].cuda_stream)
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
        _verify(bufs[k], f"stream {k + 1}")
