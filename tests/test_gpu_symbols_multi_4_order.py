"""Stream order of rs2_verifier_recovery_symbols_multi_device_async (tests/stream_order.py, used
as tests/test_gpu_order_1_calls.py uses it): both modes are issued behind a delay on the caller's
stream -- a torch stream, and torch's default stream passed as RS2_STREAM_LEGACY -- between decoys
and sentinels queued on the same stream.  Inputs: the slivers, and with CACHED the trees (device
resident, so an input like the slivers); outputs: symbols, proofs and with BUILD the trees.  The
decoys are other valid slivers with their own trees, so bytes read too early or too late show as
another sliver's symbols.  The two HOST arrays are overwritten with other valid values as soon as
the call returns.

The verifier's own stream (stream NULL) has no handle a delay could be queued on; there, three
calls are issued back to back without a synchronize between them -- a large one to keep the
stream busy, then two with different slivers into different outputs -- so the second reuses the
first's scratch while it may still be read: stream order alone must keep both right.

Two streams, one verifier: call A sits behind a delay on stream 1, call B is issued on the idle
stream 2.  B reuses A's scratch, so it must order itself after A: while the delay is pending B may
not have finished, and both results are right at the end."""
import ctypes

import numpy as np
import pytest
import torch

import symbols_multi as M
from stream_order import Delay, Input, Output, Sandwich, run_checked
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N, S_, COUNT = 100, 20, 3
MODES = ["build", "cached"]


def _targets(k):
    return [[0, k, N - 1, k - 1], [], [k + 1, 5, 5]]


def _other_targets(k):
    return [[1], [2, k + 2], [N - 2, 3, k, 4]]       # as many requests, other valid values


def _rewrite(arr, values):
    for i, x in enumerate(values):
        arr[i] = x


def _call(v, mode, counts, flat, slv, nodes, sym, prf, stream):
    return _lib.lib().rs2_verifier_recovery_symbols_multi_device_async(
        v.handle, COUNT, slv, counts, flat, _lib.RS2_TREES_CACHED if mode == "cached"
        else _lib.RS2_TREES_BUILD, nodes, sym, prf, stream)


@pytest.mark.parametrize("kind", ["stream", "legacy"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("axis", M.AXES)
def test_caller_stream(gpu, axis, mode, kind):
    dev = M.dev()
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    k = M.k_of(N, axis)
    refs = [M.reference(N, S_, axis, COUNT, seed) for seed in range(3)]
    targets, others = _targets(k), _other_targets(k)
    want_sym, want_prf = M.expected(refs[0], targets)
    slv = Input(*[r["data"] for r in refs], dev, name="d_slivers")
    sym = Output(want_sym.size, want_sym, dev, name="d_symbols")
    prf = Output(want_prf.size, want_prf, dev, name="d_proofs")
    ins, outs = [slv], [sym, prf]
    if mode == "cached":
        nodes = Input(*[r["nodes"] for r in refs], dev, name="d_nodes")
        ins.append(nodes)
    else:
        nodes = Output(refs[0]["nodes"].size, refs[0]["nodes"].reshape(-1), dev, name="d_nodes")
        outs.append(nodes)
    v = gpu.SliverVerifier(N, S_, axis)
    total = sum(len(t) for t in targets)
    a_counts, a_flat = (ctypes.c_uint32 * COUNT)(), (ctypes.c_uint16 * total)()

    def call(sw):
        _rewrite(a_counts, [len(t) for t in targets])
        _rewrite(a_flat, [t for ts in targets for t in ts])
        rc = _call(v, mode, a_counts, a_flat, slv.ptr, nodes.ptr, sym.ptr, prf.ptr,
                   ctypes.c_void_p(S.cuda_stream or 1))
        sw.mark()
        _rewrite(a_counts, [len(t) for t in others])
        _rewrite(a_flat, [t for ts in others for t in ts])
        return rc

    def check(rc):
        assert rc == 0, (rc, _lib.last_error())

    rec = run_checked(Sandwich(S, ins, outs, dev), call,
                      f"recovery_symbols_multi {axis} {mode} {kind}", check)
    assert rec["pending"]


@pytest.mark.parametrize("mode", MODES)
def test_own_stream_back_to_back(gpu, mode):
    axis = "primary"
    k = M.k_of(N, axis)
    refs = [M.reference(N, S_, axis, COUNT, seed) for seed in (0, 1)]
    big = M.reference(N, S_, axis, 64, 9)
    targets = [_targets(k), _other_targets(k)]
    v = gpu.SliverVerifier(N, S_, axis)
    L, nn = M.shape(N)
    d_big = M.to_dev(big["data"])
    big_sym = torch.zeros(64 * N * S_, dtype=torch.uint8, device=M.dev())
    big_prf = torch.zeros(64 * N * L * 32, dtype=torch.uint8, device=M.dev())
    bufs = []
    for r, ts in zip(refs, targets):
        total = sum(len(t) for t in ts)
        bufs.append((M.to_dev(r["data"]), M.to_dev(r["nodes"]) if mode == "cached" else None,
                     torch.full((total * S_,), M.FILL, dtype=torch.uint8, device=M.dev()),
                     torch.full((total * L * 32,), M.FILL, dtype=torch.uint8, device=M.dev())))
    torch.cuda.synchronize()
    assert v.recovery_symbols_multi_async(d_big.data_ptr(), [list(range(N))] * 64,
                                          big_sym.data_ptr(), big_prf.data_ptr()) == 0
    a_counts, a_flat = (ctypes.c_uint32 * COUNT)(), (ctypes.c_uint16 * 7)()
    for (d_sl, d_nodes, d_sym, d_prf), ts in zip(bufs, targets):
        _rewrite(a_counts, [len(t) for t in ts])
        _rewrite(a_flat, [t for x in ts for t in x])
        assert _call(v, mode, a_counts, a_flat, d_sl.data_ptr(),
                     d_nodes.data_ptr() if d_nodes is not None else None, d_sym.data_ptr(),
                     d_prf.data_ptr(), None) == 0, _lib.last_error()
    _rewrite(a_counts, [0, 0, 0])
    torch.cuda.synchronize()
    for (d_sl, d_nodes, d_sym, d_prf), r, ts in zip(bufs, refs, targets):
        want_sym, want_prf = M.expected(r, ts)
        assert d_sym.cpu().numpy().tobytes() == want_sym.tobytes()
        assert d_prf.cpu().numpy().tobytes() == want_prf.tobytes()
    assert big_sym.cpu().numpy().tobytes() == big["expanded"].tobytes()  # every target, in order


@pytest.mark.parametrize("mode", MODES)
def test_two_streams_one_verifier(gpu, mode):
    axis = "secondary"
    dev = M.dev()
    k = M.k_of(N, axis)
    refs = [M.reference(N, S_, axis, COUNT, seed) for seed in (0, 1)]
    targets = [_targets(k), _other_targets(k)]
    L, nn = M.shape(N)
    v = gpu.SliverVerifier(N, S_, axis)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    bufs = []
    for r, ts in zip(refs, targets):
        total = sum(len(t) for t in ts)
        bufs.append((M.to_dev(r["data"]), M.to_dev(r["nodes"]) if mode == "cached" else None,
                     torch.full((total * S_,), M.FILL, dtype=torch.uint8, device=dev),
                     torch.full((total * L * 32,), M.FILL, dtype=torch.uint8, device=dev)))

    def issue(which):
        d_sl, d_nodes, d_sym, d_prf = bufs[which]
        assert v.recovery_symbols_multi_async(
            d_sl.data_ptr(), targets[which], d_sym.data_ptr(), d_prf.data_ptr(),
            d_nodes.data_ptr() if d_nodes is not None else 0, mode,
            streams[which].cuda_stream) == 0, _lib.last_error()

    issue(0), issue(1)                       # warm-up: plans, buffers
    torch.cuda.synchronize()
    for b in bufs:
        b[2].fill_(M.FILL), b[3].fill_(M.FILL)
    torch.cuda.synchronize()
    delay = Delay(dev)
    seconds, ordered = 0.25, None
    for _ in range(3):
        gate = delay.enqueue(streams[0], seconds)
        issue(0)
        issue(1)
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
    for (d_sl, d_nodes, d_sym, d_prf), r, ts in zip(bufs, refs, targets):
        want_sym, want_prf = M.expected(r, ts)
        assert d_sym.cpu().numpy().tobytes() == want_sym.tobytes()
        assert d_prf.cpu().numpy().tobytes() == want_prf.tobytes()
