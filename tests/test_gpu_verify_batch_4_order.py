"""Stream order of rs2_decode_and_verify_batch_device_async with work pending on the stream
(tests/stream_order.py, used as tests/test_gpu_order_1_calls.py uses it): the call is issued
behind a delay, between decoys and sentinels queued on the same stream.  Inputs: slivers, pair
hashes and blob ids -- the metadata is device-resident, so it is an input like the slivers.
Outputs: the decoded blobs and the verdicts.  G3, Default, four blobs from the "pri" layout; blob
2's metadata has one bit of an unverified row's hash flipped, so the real inputs give
MATCH, MATCH, MISMATCH, MATCH while both decoys (other blobs with their own honest metadata) give
MATCH everywhere: a verdict computed from bytes read too early or too late shows.  A run whose
stream was not pending when the call returned is not a pass (run_checked)."""
import numpy as np
import pytest
import torch

import corruption as C
from stream_order import Input, Output, Sandwich, run_checked

pytestmark = pytest.mark.gpu

B = 4
MISMATCH, MATCH = 0, 1


def _set(blob, n, idx, bad_blob=None, bad_pair=None):
    """(slivers, hashes, ids) of B copies of `blob`, sliver set `idx` each."""
    prim, _, hashes, bid = C.backend(n).encode(blob, n)
    sl = np.concatenate([prim[i] for i in idx])
    hb = [bytearray(b"".join(p + q for p, q in hashes)) for _ in range(B)]
    if bad_blob is not None:
        hb[bad_blob][64 * bad_pair + 5] ^= 0x04
    return (np.concatenate([sl] * B), np.frombuffer(b"".join(bytes(h) for h in hb), np.uint8),
            np.frombuffer(bid * B, np.uint8))


@pytest.mark.parametrize("kind", ["stream", "legacy"])
def test_verified_batch_is_stream_ordered(gpu, kind):
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(dev) if kind == "stream" else torch.cuda.default_stream(dev)
    g = C.GEOMETRIES["G3"]
    axis, idx = C.layouts("G3")["pri"]
    p = C.scenario("G3").params
    unverified = max(i for i in range(p.n_primary) if i not in idx)
    real_blob = C.scenario("G3", "main").blob
    others = [np.random.default_rng(900 + k).integers(1, 256, g.length, dtype=np.uint8).tobytes()
              for k in range(2)]
    real = _set(real_blob, g.n, idx, bad_blob=2, bad_pair=unverified)
    d1, d2 = (_set(b, g.n, idx) for b in others)
    names = ("slivers", "d_hashes", "d_blob_ids")
    slv, hashes, ids = (Input(real[k], d1[k], d2[k], dev, name=names[k]) for k in range(3))
    ln = p.n_secondary * p.symbol_size
    per_blob = len(idx) * ln
    items = [(list(idx), [b * per_blob + q * ln for q in range(len(idx))]) for b in range(B)]
    stride = (g.length + 39) // 2 * 2
    sel = np.concatenate([np.arange(b * stride, b * stride + g.length) for b in range(B)])
    out = Output(B * stride, np.frombuffer(real_blob * B, np.uint8), dev, select=sel,
                 name="d_blobs_out")
    verdict = Output(B * 4, np.array([MATCH, MATCH, MISMATCH, MATCH], np.int32).view(np.uint8), dev,
                     name="d_verdict")
    plan = gpu.DevicePlan(g.n, g.length)
    assert plan.info.symbol_size == g.symbol_size

    def call(sw):
        return plan.decode_and_verify_batch_async(
            axis, items, slv.ptr, out.ptr, stride, hashes.ptr, ids.ptr, "default", verdict.ptr,
            stream=S.cuda_stream or 1, statuses=True)

    def check(codes):
        assert codes == [0] * B, codes

    rec = run_checked(Sandwich(S, [slv, hashes, ids], [out, verdict], dev), call,
                      f"decode_and_verify_batch_async G3 default {kind}", check)
    assert rec["pending"]
