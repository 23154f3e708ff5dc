"""Stream order of rs2_sliver_checker_recovery_symbols_device_async (tests/stream_order.py, used as
tests/test_gpu_symbols_multi_4_order.py uses it): both modes are issued behind a delay on the
caller's stream -- a torch stream, and torch's default stream passed as RS2_STREAM_LEGACY --
between decoys and sentinels queued on the same stream.  Inputs: the slivers, and with CACHED the
trees; outputs: symbols, proofs and with BUILD the trees.  The decoys are other valid slivers of
the same sizes with their own trees, so bytes read too early or too late show as another sliver's
symbols.  The HOST arrays are overwritten with other values as soon as the call returns
(symbols_mixed.call_raw).

Back to back on the checker's own stream: a mixed call, a mixed verification and another mixed
call with other slivers, no synchronize between them -- the verification reuses the gathered,
repair and table buffers, so stream order alone must keep all three right.

Two streams, one checker: call A sits behind a delay on stream 1, call B is issued on the idle
stream 2.  B reuses A's scratch, so it must order itself after A."""
import numpy as np
import pytest
import torch

import symbols_mixed as X
import verify_mixed as VM
from stream_order import Delay, Input, Output, Sandwich, run_checked
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 100


def _items(shift=0):
    out = []
    for q, (a, s) in enumerate([("primary", 6), ("secondary", 18), ("primary", 2), ("secondary", 6),
                                ("primary", 6)]):
        k = X.k_of(N, a)
        ts = [[0, k, N - 1, k - 1], [3, 1], [k + 1, 5, 5], [], [k, 0]][q]
        out.append((a, s, (q + shift) % X.POOL, ts))
    return out


def _nodes(items):
    return np.concatenate([np.frombuffer(w[2], dtype=np.uint8) for w in X.want(N, items)])


@pytest.mark.parametrize("kind", ["stream", "legacy"])
@pytest.mark.parametrize("mode", ["build", "cached"])
def test_caller_stream(gpu, mode, kind):
    dev = X.dev()
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    variants = [_items(shift) for shift in range(3)]
    items = variants[0]
    L, nn = X.shape(N)
    i_off, i_size, o_off, o_size = X.layout(N, items, out_gap=0)
    wants = X.want(N, items)
    want_sym = np.frombuffer(b"".join(w[0] for w in wants), dtype=np.uint8)
    want_prf = np.frombuffer(b"".join(w[1] for w in wants), dtype=np.uint8)
    assert want_sym.size == o_size
    slv = Input(*[X.payload(N, v, i_off, i_size) for v in variants], dev, name="d_slivers")
    sym = Output(want_sym.size, want_sym, dev, name="d_symbols")
    prf = Output(want_prf.size, want_prf, dev, name="d_proofs")
    ins, outs = [slv], [sym, prf]
    if mode == "cached":
        nodes = Input(*[_nodes(v) for v in variants], dev, name="d_nodes")
        ins.append(nodes)
    else:
        nodes = Output(len(items) * nn * 32, _nodes(items), dev, name="d_nodes")
        outs.append(nodes)
    c = gpu.SliverChecker(N)

    def call(sw):
        rc = X.call_raw(c, items, slv.ptr, i_off, sym.ptr, o_off, prf.ptr, nodes.ptr, mode,
                        S.cuda_stream or 1)
        sw.mark()
        return rc

    def check(rc):
        assert rc == 0, (rc, _lib.last_error())

    rec = run_checked(Sandwich(S, ins, outs, dev), call, f"symbols_mixed {mode} {kind}", check)
    assert rec["pending"]


def _buffers(items, mode):
    L, nn = X.shape(N)
    i_off, i_size, o_off, o_size = X.layout(N, items)
    total = sum(len(it[3]) for it in items)
    dev = X.dev()
    return {"items": items, "i_off": i_off, "o_off": o_off,
            "sl": X.to_dev(X.payload(N, items, i_off, i_size)),
            "nodes": X.to_dev(_nodes(items)) if mode == "cached"
            else torch.full((len(items) * nn * 32,), X.FILL, dtype=torch.uint8, device=dev),
            "sym": torch.full((o_size,), X.FILL, dtype=torch.uint8, device=dev),
            "prf": torch.full((total * L * 32,), X.FILL, dtype=torch.uint8, device=dev)}


def _issue(c, b, mode, stream=None):
    assert X.call_raw(c, b["items"], b["sl"].data_ptr(), b["i_off"], b["sym"].data_ptr(), b["o_off"],
                      b["prf"].data_ptr(), b["nodes"].data_ptr(), mode, stream) == 0, _lib.last_error()


def _verify(b, mode):
    X.check_outputs(N, b["items"], b["sym"].cpu().numpy(), b["o_off"], b["prf"].cpu().numpy(),
                    b["nodes"].cpu().numpy(), what=mode)


@pytest.mark.parametrize("mode", ["build", "cached"])
def test_own_stream_back_to_back_with_a_verification_between(gpu, mode):
    c = gpu.SliverChecker(N)
    bufs = [_buffers(_items(shift), mode) for shift in (0, 1)]
    # the verification between them: other sizes, so the tables and scratch are laid out anew
    v_items = [(a, s, seed) for seed, (a, s) in enumerate([("primary", 20), ("secondary", 4),
                                                            ("primary", 66)])]
    v_off, at = [], 0
    for a, s, _ in v_items:
        v_off.append(at)
        at += X.k_of(N, a) * s
    v_data = X.to_dev(np.concatenate([VM.sliver(N, s, a, seed) for a, s, seed in v_items]))
    d_roots = torch.full((3 * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
    torch.cuda.synchronize()
    _issue(c, bufs[0], mode)
    assert c.verify_async([a for a, _, _ in v_items], [s for _, s, _ in v_items], v_data.data_ptr(),
                          v_off, None, d_roots.data_ptr()) == 0, _lib.last_error()
    _issue(c, bufs[1], mode)
    torch.cuda.synchronize()
    for b in bufs:
        _verify(b, mode)
    assert d_roots.cpu().numpy().tobytes() == b"".join(VM.root(N, s, a, seed) for a, s, seed in v_items)


@pytest.mark.parametrize("mode", ["build", "cached"])
def test_two_streams_one_checker(gpu, mode):
    dev = X.dev()
    c = gpu.SliverChecker(N)
    bufs = [_buffers(_items(shift), mode) for shift in (0, 1)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]

    def issue(which):
        _issue(c, bufs[which], mode, streams[which].cuda_stream)

    issue(0), issue(1)                       # warm-up: codes, buffers
    torch.cuda.synchronize()
    for b in bufs:
        b["sym"].fill_(X.FILL), b["prf"].fill_(X.FILL)
        if mode == "build":
            b["nodes"].fill_(X.FILL)
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
    for b in bufs:
        _verify(b, mode)
