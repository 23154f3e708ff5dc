"""rs2_decode_and_verify_batch_device_async inside guard bands (tests/guarded.py): every buffer
of the call is the interior of a larger patterned allocation, the symbol buffers (slivers, decoded
blobs) at every even placement mod 16, the digest and verdict buffers 16-byte aligned, and
out_stride is larger than any blob.  Nothing outside the stated extents may change: the guards,
the inputs, the stride gaps and every byte at or past a blob's length.  A second run with another
guard fill around every input must give bit-identical outputs and verdicts: no result depends on
a byte outside an input's extent (the gather reads up to a row's valid end and no further)."""
import numpy as np
import pytest
import torch

import corruption as C
import verify_batch as VB
from guarded import DELTAS, Guarded

pytestmark = pytest.mark.gpu


def _run(plan, packed, check, delta, fill, stride):
    dev = torch.device("cuda", 0)
    B = len(packed.blobs)
    slivers = Guarded(packed.slivers.size, delta, dev, fill).set(packed.slivers)
    hashes = Guarded(packed.hashes.size, 0, dev, fill + 1).set(packed.hashes)
    ids = Guarded(packed.ids.size, 0, dev, fill + 2).set(packed.ids)
    out = Guarded(B * stride, delta, dev, 77)
    verdict = Guarded(B * 4, 0, dev, 78)
    torch.cuda.synchronize()
    st = plan.decode_and_verify_batch_async(
        packed.axis, packed.blobs, slivers.ptr, out.ptr, stride, hashes.ptr, ids.ptr, check,
        verdict.ptr, blob_lens=packed.lens, statuses=True)
    plan.sync()
    torch.cuda.synchronize()
    assert st == [0] * B
    for g, data, what in ((slivers, packed.slivers, "slivers"), (hashes, packed.hashes, "hashes"),
                          (ids, packed.ids, "blob ids")):
        g.assert_guards_intact(what=what)
        assert g.numpy().tobytes() == data.tobytes(), what + " were written"
    out.assert_guards_intact([(b * stride, ln) for b, ln in enumerate(packed.lens)], "d_blobs_out")
    verdict.assert_guards_intact(what="d_verdict")
    return out.numpy().reshape(B, stride), verdict.numpy().view(np.int32).copy()


@pytest.mark.parametrize("check", ["default", "strict"])
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", ["G2", "G3"])
def test_inside_guards(gpu, gid, axis, delta, check):
    g = C.GEOMETRIES[gid]
    cases = VB.batch_cases(gid, axis, check)[:40]
    want = VB.model_verdicts(cases)
    plan = gpu.DevicePlan(g.n, g.length)
    packed = VB.pack(cases)
    stride = (g.length + 51) // 2 * 2
    out, verdicts = _run(plan, packed, check, delta, 11, stride)
    for b, (c, w) in enumerate(zip(cases, want)):
        assert verdicts[b] == (VB.MATCH if w[0] == "ok" else VB.MISMATCH), c.describe()
        if w[0] == "ok":
            assert out[b, :packed.lens[b]].tobytes() == w[1], c.describe()
    out2, verdicts2 = _run(plan, packed, check, delta, 151, stride)
    assert (verdicts2 == verdicts).all()
    for b, ln in enumerate(packed.lens):
        assert (out2[b, :ln] == out[b, :ln]).all(), b
