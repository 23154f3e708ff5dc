"""Sliver verification under corruption: verify_slivers / sliver_merkle_roots (host buffers,
pooled verifiers) and SliverVerifier.roots_async (device buffers), batch by batch.

Every root must be the oracle's root of the sliver AS CORRUPTED (single-bit flips at the byte
positions of corruption.sliver_positions), every boolean false exactly for the corrupted
members.  Each batch runs honest, corrupt, honest, corrupt (another member), honest, on the same
verifier and in the same buffers, so a root or a verdict replayed from the previous call shows.
Trees run four per workgroup, one wave each: batch sizes 1, 3, 4, 5, 65 and n, with the first,
the last, the last but one and a member with index % 4 == 3 corrupted.
"""
from itertools import cycle

import numpy as np
import pytest

import corruption as C

pytestmark = pytest.mark.gpu

GEOS = ["G1", "G3", "G4", "G5"]


def _members(count):
    """Corrupt members of the first corrupt batch, and the one of the second."""
    first = sorted({0, count - 1, max(count - 2, 0)} |
                   ({max(i for i in range(count) if i % 4 == 3)} if count > 3 else set()))
    second = next((i for i in (count // 2, 1, 0) if i < count and i not in first), 0)
    return first, [second]


def _batches(gid, axis):
    """[(count, honest slivers [(index, bytes)], [corrupt batch {member: (byte, mask)}, ...])]."""
    sc = C.scenario(gid)
    n = sc.geo.n
    pos = cycle(C.sliver_positions(sc.params, axis))
    out = []
    for count in sorted({1, 3, 4, 5, 65, n}):
        idx = [(7 * j + count) % n for j in range(count)]   # repeats where count > n
        honest = [(i, sc.sliver(axis, i)) for i in idx]
        first, second = _members(count)
        a = {m: next(pos) for m in first}
        b = {m: next(pos) for m in second}
        if b == a:   # count == 1: the one member again, at another byte
            b = {m: next(pos) for m in second}
        out.append((count, honest, [a, b]))
    return out


def _apply(honest, flips):
    batch = list(honest)
    for m, (byte, mask) in flips.items():
        d = bytearray(batch[m][1])
        d[byte] ^= mask
        batch[m] = (batch[m][0], bytes(d))
    return batch


def _want_roots(sc, axis, honest, flips):
    roots = [sc.hashes[sc.pair_of(axis, i)][axis == C.SECONDARY] for i, _ in honest]
    for m, (i, d) in enumerate(_apply(honest, flips)):
        if m in flips:
            roots[m] = C.sliver_root(sc.params, axis, d)
            assert roots[m] != sc.hashes[sc.pair_of(axis, i)][axis == C.SECONDARY]
    return roots


@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", GEOS)
def test_verify_slivers_host(gpu, gid, axis):
    from walrus_amd.encoding import sliver_merkle_roots
    sc = C.scenario(gid)
    g = sc.geo
    cfg = gpu.ReedSolomonEncodingConfig(g.n)
    assert cfg.symbol_size_for_blob(g.length) == g.symbol_size
    md = gpu.BlobMetadata(sc.hashes, g.length)

    def run(honest, flips):
        slivers = [gpu.SliverData(gpu.Symbols(d, g.symbol_size), i, axis)
                   for i, d in _apply(honest, flips)]
        what = (gid, axis, len(honest), flips)
        assert sliver_merkle_roots(cfg, slivers) == _want_roots(sc, axis, honest, flips), what
        assert gpu.verify_slivers(cfg, md, slivers) == \
            [m not in flips for m in range(len(honest))], what
        for m in sorted(flips)[:2]:
            with pytest.raises(gpu.VerificationError):
                slivers[m].verify(cfg, md)
        good = next((m for m in range(len(honest)) if m not in flips), None)
        if good is not None:
            slivers[good].verify(cfg, md)

    for count, honest, (a, b) in _batches(gid, axis):
        for flips in ({}, a, {}, b, {}):
            run(honest, flips)


@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", GEOS)
def test_roots_async_device(gpu, gid, axis):
    """One SliverVerifier, one sliver buffer and one root buffer for every batch of the
    geometry; flips are XORed in place and taken out again; the batches alternate between the
    null stream and a torch stream."""
    import torch
    dev = torch.device("cuda", 0)
    sc = C.scenario(gid)
    g = sc.geo
    ln = len(sc.sliver(axis, 0))
    batches = _batches(gid, axis)
    most = max(count for count, _, _ in batches)
    buf = torch.zeros(most * ln + 256, dtype=torch.uint8, device=dev)
    roots = torch.zeros(most * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    v = gpu.SliverVerifier(g.n, g.symbol_size, axis)
    side = torch.cuda.Stream(dev)
    for k, (count, honest, (a, b)) in enumerate(batches):
        use_side = k % 2 == 1
        with torch.cuda.stream(side if use_side else None):
            host = np.frombuffer(b"".join(d for _, d in honest), np.uint8)
            buf[:host.size].copy_(torch.from_numpy(host.copy()))
            for flips in ({}, a, {}, b, {}):
                for m, (byte, mask) in flips.items():
                    buf[m * ln + byte:m * ln + byte + 1] ^= mask
                roots.fill_(0xEE)
                v.roots_async(count, buf.data_ptr(), roots.data_ptr(),
                              side.cuda_stream if use_side else 0)
                got = roots.cpu().numpy().tobytes()
                for m, (byte, mask) in flips.items():
                    buf[m * ln + byte:m * ln + byte + 1] ^= mask
                want = _want_roots(sc, axis, honest, flips)
                assert [got[32 * m:32 * m + 32] for m in range(count)] == want, \
                    (gid, axis, count, flips)
                assert got[32 * count:] == b"\xee" * (32 * (most - count))
            assert buf[:host.size].cpu().numpy().tobytes() == host.tobytes()
