"""decode_and_verify under corruption against the oracle model (tests/corruption.py), through the
host mirror and through the device entry point.

Every case is one single-bit change of a sliver, a metadata hash, the blob id or the length;
the model decides the verdict and, on accept, every returned byte.  Honest calls are woven in
(corruption.run_sequence), on the same plan, the same device addresses and the same stream, so
a verdict path that reads what the previous call left behind -- check_roots, check_rows,
dev_blob, the plan's blob id, a pooled verifier's buffers, a decode slot reused for an
identical key -- fails here while every honest-data test still passes.
"""
import numpy as np
import pytest

import corruption as C

pytestmark = pytest.mark.gpu


def _engine_encode(gpu, gid, scen="main"):
    """The engine's own encode of the scenario, asserted equal to the oracle's."""
    sc = C.scenario(gid, scen)
    cfg = _config(gpu, gid)
    assert cfg.symbol_size_for_blob(sc.geo.length) == sc.geo.symbol_size
    pairs, meta = cfg.encode_with_metadata(sc.blob)
    n = sc.geo.n
    assert bytes(meta.blob_id) == sc.blob_id
    assert meta.metadata.hashes == sc.hashes
    for i in range(n):
        assert pairs[i].primary.symbols.data == sc.primary[i].tobytes(), i
        assert pairs[i].secondary.index == n - 1 - i
        assert pairs[i].secondary.symbols.data == sc.secondary[n - 1 - i].tobytes(), i
    return sc


_CONFIGS = {}


def _config(gpu, gid):
    """One ReedSolomonEncodingConfig per geometry: one cached plan for every call."""
    if gid not in _CONFIGS:
        _CONFIGS[gid] = gpu.ReedSolomonEncodingConfig(C.GEOMETRIES[gid].n)
    return _CONFIGS[gid]


@pytest.mark.parametrize("gid", list(C.GEOMETRIES))
def test_host_mirror(gpu, gid):
    cfg = _config(gpu, gid)
    s = C.GEOMETRIES[gid].symbol_size
    cases = C.cases(gid)
    for scen in sorted({c.scen for c in cases}):
        _engine_encode(gpu, gid, scen)

    def call(case):
        m = C.materialise(case)
        slivers = [gpu.SliverData(gpu.Symbols(d, s), i, m["axis"]) for i, d in m["slivers"]]
        meta = gpu.VerifiedBlobMetadataWithId(gpu.BlobId(m["blob_id"]),
                                              gpu.BlobMetadata(m["hashes"], m["length"]))
        try:
            return ("ok", cfg.decode_and_verify(meta, slivers, m["check"]))
        except gpu.VerificationError:
            return ("rejected",)

    plans = set()
    total = {"ok": 0, "rejected": 0, "honest": 0}
    for _, group in C.groups(cases):
        for k, v in C.run_sequence(call, group).items():
            total[k] += v
        plans.add(id(cfg._plan(C.GEOMETRIES[gid].length)))
    assert len(plans) == 1 and len(cfg._plans) == 1   # every call went through one plan
    print(gid, "host", total)


@pytest.mark.parametrize("stream_kind", ["own", "legacy", "torch"])
@pytest.mark.parametrize("gid", ["G0_1", "G1", "G2", "G3", "G4", "G5"])
def test_device_entry_point(gpu, gid, stream_kind):
    """rs2_decode_and_verify_device on one DevicePlan and one set of device buffers: each case
    XORs its bit in place in the sliver buffer and takes it out again, so base, offsets and the
    output address never change and a decode slot is reused with an identical key while the
    content differs.  The flip and the call are ordered by the stream alone (for the plan's own
    stream: by a wait on the stream that wrote the flip); nothing waits for the whole device."""
    import torch
    dev = torch.device("cuda", 0)
    g = C.GEOMETRIES[gid]
    cases = [c for c in C.cases(gid) if not (g.length + c.dlen == 0)]
    plan = gpu.DevicePlan(g.n, g.length)
    info = plan.info
    assert info.symbol_size == g.symbol_size
    lens = {C.PRIMARY: info.primary_sliver_len, C.SECONDARY: info.secondary_sliver_len}
    most = max(len(idx) * lens[axis] for axis, idx in C.layouts(gid).values())
    buf = torch.zeros(most + 256, dtype=torch.uint8, device=dev)
    out = torch.zeros(g.length + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)   # the buffers exist before another stream touches them
    side = torch.cuda.Stream(dev)
    st = {"own": None, "legacy": 0, "torch": side.cuda_stream}[stream_kind]
    ctx = torch.cuda.stream(side) if stream_kind == "torch" else torch.cuda.stream(None)

    def call(case):
        sc = C.scenario(case.geo, case.scen)
        axis, idx = C.layouts(gid)[case.layout]
        ln = lens[axis]
        hashes, bid = list(sc.hashes), bytearray(sc.blob_id)
        if case.hash_edit:
            pair, which, b, m = case.hash_edit
            h = [bytearray(x) for x in hashes[pair]]
            h[which][b] ^= m
            hashes[pair] = (bytes(h[0]), bytes(h[1]))
        if case.id_edit:
            bid[case.id_edit[0]] ^= case.id_edit[1]
        length = g.length + case.dlen
        plan._plan.bind(length)
        cell = buf[case.pos * ln + case.byte:case.pos * ln + case.byte + 1] if case.pos >= 0 \
            else None
        out.fill_(0xEE)
        if cell is not None:
            cell ^= case.mask
        if st is None:
            torch.cuda.current_stream(dev).synchronize()
        try:
            plan.decode_and_verify(axis, list(idx), buf.data_ptr(),
                                   [i * ln for i in range(len(idx))],
                                   b"".join(p + q for p, q in hashes), bytes(bid), case.check,
                                   out.data_ptr(), st)
            got = out.cpu().numpy()
            assert (got[length:] == 0xEE).all(), "wrote past the blob: " + case.describe()
            res = ("ok", got[:length].tobytes())
        except gpu.VerificationError:
            res = ("rejected",)
        finally:
            if cell is not None:
                cell ^= case.mask
        return res

    total = {"ok": 0, "rejected": 0, "honest": 0}
    with ctx:
        for (scen, layout), group in C.groups(cases):
            sc = C.scenario(gid, scen)
            axis, idx = C.layouts(gid)[layout]
            host = np.concatenate([np.frombuffer(sc.sliver(axis, i), np.uint8) for i in idx])
            buf[:host.size].copy_(torch.from_numpy(host.copy()))
            for k, v in C.run_sequence(call, group).items():
                total[k] += v
            # the buffer is honest again after the last case
            assert buf[:host.size].cpu().numpy().tobytes() == host.tobytes()
    print(gid, stream_kind, total)
