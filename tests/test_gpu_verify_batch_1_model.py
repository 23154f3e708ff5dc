"""rs2_decode_and_verify_batch_device_async / rs2_decode_and_verify_batch against the oracle
model (tests/corruption.py), many corruption cases per call.

One batched call holds every case of a geometry, axis and check (tests/verify_batch.py): all
layouts, both scenarios, each blob with its own length, the layout's honest case after every
fourth one -- honest and corrupted blobs side by side in the same launches, which a per-blob loop
can never test.  Every Default and Strict call of the table in tests/test_verify_plan.py holds
both verdicts, so a path that answers all-MATCH or all-MISMATCH fails.

Stale state: a second call on the same buffers with every blob honest must give all MATCH, a
third with the corruptions back the first call's verdicts again.
"""
import numpy as np
import pytest

import corruption as C
import verify_batch as VB

pytestmark = pytest.mark.gpu

GIDS = ["G0_1", "G1", "G2", "G3", "G4", "G5"]


@pytest.mark.parametrize("check", C.CHECKS)
@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", GIDS)
def test_device_batch(gpu, gid, axis, check):
    from walrus_amd.encoding import decode_batch_stats
    g = C.GEOMETRIES[gid]
    cases = VB.batch_cases(gid, axis, check)
    want = VB.model_verdicts(cases)
    if check == "skip":
        assert all(w[0] == "ok" for w in want)
    plan = gpu.DevicePlan(g.n, g.length)
    assert plan.info.symbol_size == g.symbol_size
    packed = VB.pack(cases)
    honest = VB.pack(cases, honest=True)
    assert honest.slivers.size == packed.slivers.size and honest.blobs == packed.blobs
    call = VB.DeviceCall(gpu, plan, packed)
    B = len(cases)

    before = decode_batch_stats()
    verdicts, out, st = call.run(packed, check, statuses=True)
    after = decode_batch_stats()
    assert st == [0] * B
    VB.assert_against_model(cases, want, verdicts, out, packed.lens, "first call")
    if g.symbol_size == 2:   # no batch job at a 2-byte symbol: every blob decodes on its own
        assert after["batched"] == before["batched"]
        assert after["single"] - before["single"] == B
    else:
        assert after["batched"] > before["batched"] and after["launches"] > before["launches"]

    # every blob honest, same buffers: nothing of the first call may show
    verdicts2, out2, _ = call.run(honest, check)
    assert (verdicts2 == VB.MATCH).all(), np.nonzero(verdicts2 != VB.MATCH)[0]
    for b, c in enumerate(cases):
        blob = C.scenario(c.geo, c.scen).blob
        assert out2[b, :len(blob)].tobytes() == blob, b
        assert (out2[b, len(blob):] == VB.OUT_FILL).all(), b

    # the corruptions back: the first call's verdicts and bytes again
    verdicts3, out3, _ = call.run(packed, check)
    assert (verdicts3 == verdicts).all()
    VB.assert_against_model(cases, want, verdicts3, out3, packed.lens, "third call")
    print(gid, axis, check, B, "blobs,", int((verdicts == VB.MATCH).sum()), "match")


@pytest.mark.parametrize("check", C.CHECKS)
@pytest.mark.parametrize("gid", ["G1", "G3", "G4"])
def test_host_form(gpu, gid, check):
    """ReedSolomonEncodingConfig.decode_and_verify_batch: both axes in one call (the mirror
    groups them), the blob per item or None where the model rejects."""
    g = C.GEOMETRIES[gid]
    cfg = gpu.ReedSolomonEncodingConfig(g.n)
    s = g.symbol_size
    cases = VB.batch_cases(gid, C.PRIMARY, check) + VB.batch_cases(gid, C.SECONDARY, check)
    want = VB.model_verdicts(cases)
    items = []
    for c in cases:
        m = C.materialise(c)
        slivers = [gpu.SliverData(gpu.Symbols(d, s), i, m["axis"]) for i, d in m["slivers"]]
        items.append((gpu.VerifiedBlobMetadataWithId(gpu.BlobId(m["blob_id"]),
                                                     gpu.BlobMetadata(m["hashes"], m["length"])),
                      slivers))
    got = cfg.decode_and_verify_batch(items, check)
    assert len(got) == len(cases)
    for b, (c, w) in enumerate(zip(cases, want)):
        if w[0] == "ok":
            assert got[b] == w[1], f"blob {b}: {c.describe()}"
        else:
            assert got[b] is None, f"blob {b} accepted, the model rejects: {c.describe()}"
    assert any(x is None for x in got) == (check != "skip")
