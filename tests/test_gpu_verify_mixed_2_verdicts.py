"""Verdicts of the mixed sliver verification (rs2_sliver_checker_verify_device_async,
rs2_verify_slivers_mixed) under corruption.  On one checker and the same device buffers the
sequence honest, corrupt, honest, corrupt, honest runs over groups of three slivers: the corrupt
rounds flip single bits (corruption.sliver_positions: the first, a middle and the last symbol x
the symbol's edge offsets) in the first member of one group, the last member of another and the
middle member of a third, then in other members.  Every root must be the oracle's root of the
sliver as corrupted, and RS2_SLIVER_MISMATCH must appear exactly at the corrupt members: a group
launch that mixed lines up, or reused a stale gathered copy, shows here.

Refusals: one of each per-sliver rule is RS2_SLIVER_SKIPPED with its code in status_out and its
root slot left alone; without status_out the first failing code is returned and nothing is
written.  The host form gives the same verdicts.

verify_slivers_of_blobs runs over real blobs of different symbol sizes and must agree with
verify_slivers per blob.  A call is bound to one n_shards, so the three blobs of the n = 10 call are
corruption.scenario("G1") (s = 6), scenario("G3")'s blob bytes encoded at n = 10 (s = 104) and the
one-byte blob of "G0_1" (s = 2, the per-size path); scenario("G3") itself (n = 13, s = 66) runs
beside a second n = 13 blob in a call of its own."""
import ctypes

import numpy as np
import pytest
import torch

import corruption
import verify_mixed as M
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

INVALID, INCOMPATIBLE = _lib.RS2_E_INVALID_ARGUMENT, _lib.RS2_E_INCOMPATIBLE_PARAMETERS
BAD_LENGTH = _lib.RS2_E_INCORRECT_DATA_LENGTH


def _flip(n, items, i, which):
    """Item i's sliver with one bit flipped at sliver_positions[which]."""
    a, s, seed = items[i]
    pos = corruption.sliver_positions(M.params(n, s), a)
    byte, mask = pos[which % len(pos)]
    d = bytearray(M.sliver(n, s, a, seed).tobytes())
    d[byte] ^= mask
    return bytes(d)


@pytest.mark.parametrize("n,sizes", [(13, [4, 6, 66, 130]), (100, [6, 64, 258]),
                                     (1000, [20, 130])])
def test_honest_corrupt_sequence(gpu, n, sizes):
    items = M.groups_case(n, sizes, 3, "interleaved")
    m = len(items)
    groups = [(a, s) for s in sizes for a in M.AXES]
    member = lambda g, j: [i for i, it in enumerate(items) if (it[0], it[1]) == groups[g]][j]
    rounds = [
        {},
        {member(0, 0): 0, member(1, 2): 3, member(len(groups) - 1, 1): 7},
        {},
        {member(2 % len(groups), 1): 11, member(0, 2): 5, member(len(groups) - 1, 0): 2},
        {},
    ]
    off, size = M.layout(n, items)
    expected = M.expected_roots(n, items)
    checker = gpu.SliverChecker(n)
    d_in = torch.zeros(size, dtype=torch.uint8, device=M.dev())
    d_roots = torch.zeros(m * 32, dtype=torch.uint8, device=M.dev())
    d_verdict = torch.zeros(m, dtype=torch.int32, device=M.dev())
    for r, flips in enumerate(rounds):
        data = [_flip(n, items, i, flips[i]) if i in flips else None for i in range(m)]
        d_in.copy_(torch.tensor(M.payload(n, items, off, size, data)))
        d_roots.fill_(M.FILL)
        d_verdict.fill_(-1)
        torch.cuda.synchronize()
        rc = checker.verify_async([a for a, _, _ in items], [s for _, s, _ in items],
                                  d_in.data_ptr(), off, expected, d_roots.data_ptr(),
                                  d_verdict.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.last_error())
        M.check_roots(n, items, d_roots.cpu().numpy().tobytes(), data, f"n={n} round {r}")
        want = [M.MISMATCH if i in flips else M.MATCH for i in range(m)]
        assert d_verdict.cpu().tolist() == want, f"round {r}"
        # the host form: the same verdicts and roots
        keep = [np.frombuffer(data[i], dtype=np.uint8) if data[i] is not None
                else M.sliver(n, *reversed(items[i][:2]), items[i][2]) for i in range(m)]
        h_roots, h_verdict = _host_call(n, items, keep, expected)[1:3]
        assert h_verdict == want and h_roots == d_roots.cpu().numpy().tobytes()


def _host_call(n, items, keep, expected, status=False, axes=None, sizes=None, lens=None,
               null=()):
    m = len(items)
    axes = axes if axes is not None else [_lib.AXIS_PRIMARY if a == "primary"
                                          else _lib.AXIS_SECONDARY for a, _, _ in items]
    sizes = sizes if sizes is not None else [s for _, s, _ in items]
    lens = lens if lens is not None else [len(k) for k in keep]
    ptrs = (ctypes.c_void_p * m)(*[None if i in null else keep[i].ctypes.data for i in range(m)])
    roots = np.full(m * 32, M.FILL, dtype=np.uint8)
    verdict = np.full(m, -1, dtype=np.int32) if expected is not None else None
    st = (ctypes.c_int * m)(*([-1] * m)) if status else None
    exp = np.frombuffer(expected, dtype=np.uint8) if expected is not None else None
    rc = _lib.lib().rs2_verify_slivers_mixed(
        n, m, (ctypes.c_uint8 * m)(*axes), (ctypes.c_uint16 * m)(*sizes), ptrs,
        (ctypes.c_uint64 * m)(*lens), exp.ctypes.data if exp is not None else None,
        roots.ctypes.data, verdict.ctypes.data if verdict is not None else None, st)
    return (rc, roots.tobytes(), verdict.tolist() if verdict is not None else None,
            list(st) if status else None)


def test_refusals_are_skipped(gpu):
    """Device form: a bad axis, a zero and an odd symbol size, an odd offset -- between good
    slivers of both paths (s = 2: per-size, the others: group launches)."""
    n = 13
    items = [("primary", 6, 0), ("secondary", 66, 1), ("primary", 2, 0), ("secondary", 6, 2),
             ("primary", 130, 3), ("secondary", 4, 0), ("primary", 66, 1), ("secondary", 2, 1)]
    m = len(items)
    off, size = M.layout(n, items)
    axes = [M.AXES.index(a) for a, _, _ in items]
    sizes = [s for _, s, _ in items]
    offs = list(off)
    axes[1], sizes[3], sizes[4], offs[5] = 2, 0, 129, off[5] + 1
    want_status = [0, INVALID, 0, INCOMPATIBLE, INCOMPATIBLE, INVALID, 0, 0]
    good = [i for i in range(m) if want_status[i] == 0]
    expected = M.expected_roots(n, items)
    checker = gpu.SliverChecker(n)
    d_in = torch.tensor(M.payload(n, items, off, size), dtype=torch.uint8, device=M.dev())
    d_roots = torch.full((m * 32,), M.FILL, dtype=torch.uint8, device=M.dev())
    d_verdict = torch.full((m,), -1, dtype=torch.int32, device=M.dev())
    torch.cuda.synchronize()
    # without status_out: the first failing code, nothing enqueued, nothing written
    before = M.stats()
    rc = M.call(checker, axes, sizes, d_in.data_ptr(), offs,
                np.frombuffer(expected, dtype=np.uint8).ctypes.data, d_roots.data_ptr(),
                d_verdict.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == INVALID and M.moved(before) == [0] * 5
    assert bool((d_roots == M.FILL).all()) and bool((d_verdict == -1).all())
    # with it: the refused ones are skipped, the rest run
    status = (ctypes.c_int * m)(*([-1] * m))
    rc = M.call(checker, axes, sizes, d_in.data_ptr(), offs,
                np.frombuffer(expected, dtype=np.uint8).ctypes.data, d_roots.data_ptr(),
                d_verdict.data_ptr(), status)
    torch.cuda.synchronize()
    assert rc == 0 and list(status) == want_status
    roots = d_roots.cpu().numpy().tobytes()
    for i in range(m):
        if i in good:
            assert roots[32 * i:32 * i + 32] == expected[32 * i:32 * i + 32], i
        else:
            assert roots[32 * i:32 * i + 32] == bytes([M.FILL]) * 32, i
    assert d_verdict.cpu().tolist() == [M.MATCH if i in good else M.SKIPPED for i in range(m)]
    # every sliver refused: verdicts only
    d_verdict.fill_(-1)
    status = (ctypes.c_int * 2)(-1, -1)
    rc = M.call(checker, [5, 0], [4, 3], d_in.data_ptr(), [0, 0],
                np.frombuffer(expected, dtype=np.uint8).ctypes.data, d_roots.data_ptr(),
                d_verdict.data_ptr(), status)
    torch.cuda.synchronize()
    assert rc == 0 and list(status) == [INVALID, INCOMPATIBLE]
    assert d_verdict.cpu().tolist()[:3] == [M.SKIPPED, M.SKIPPED, -1]


def test_host_form_refusals(gpu):
    n = 10
    items = [("primary", 6, 0), ("secondary", 6, 0), ("primary", 64, 1), ("secondary", 2, 0),
             ("primary", 4, 2)]
    m = len(items)
    keep = [M.sliver(n, s, a, seed) for a, s, seed in items]
    expected = M.expected_roots(n, items)
    lens = [len(k) for k in keep]
    lens[2] -= 2
    want_status = [0, BAD_LENGTH, BAD_LENGTH, 0, 0]
    rc, roots, verdict, status = _host_call(n, items, keep, expected, status=True, lens=lens,
                                            null=(1,))
    assert rc == 0 and status == want_status
    assert verdict == [M.MATCH, M.SKIPPED, M.SKIPPED, M.MATCH, M.MATCH]
    for i in range(m):
        want = expected[32 * i:32 * i + 32] if want_status[i] == 0 else bytes([M.FILL]) * 32
        assert roots[32 * i:32 * i + 32] == want, i
    # without status_out the first failing code comes back and the outputs stay untouched
    rc, roots, verdict, _ = _host_call(n, items, keep, expected, lens=lens, null=(1,))
    assert rc == BAD_LENGTH and roots == bytes([M.FILL]) * (32 * m) and verdict == [-1] * m
    # whole-call rules of the host form
    assert _host_call(n, items, keep, None)[0] == 0
    exp = np.frombuffer(expected, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * m)(*[k.ctypes.data for k in keep])
    ax = (ctypes.c_uint8 * m)(*[M.AXES.index(a) for a, _, _ in items])
    sz = (ctypes.c_uint16 * m)(*[s for _, s, _ in items])
    ln = (ctypes.c_uint64 * m)(*[len(k) for k in keep])
    out = np.zeros(m * 32, dtype=np.uint8)
    lib = _lib.lib()
    assert lib.rs2_verify_slivers_mixed(n, m, ax, sz, ptrs, ln, exp.ctypes.data, out.ctypes.data,
                                        None, None) == INVALID     # expected without verdicts
    assert lib.rs2_verify_slivers_mixed(n, m, None, sz, ptrs, ln, None, out.ctypes.data, None,
                                        None) == INVALID
    assert lib.rs2_verify_slivers_mixed(n, 65536, ax, sz, ptrs, ln, None, out.ctypes.data, None,
                                        None) == INVALID
    assert lib.rs2_verify_slivers_mixed(n, 0, None, None, None, None, None, None, None, None) == 0


def _blob_slivers(gpu, n, hashes, length, primary, secondary, s):
    meta = gpu.BlobMetadata(list(hashes), length)
    slivers = []
    for i in range(n):
        slivers.append(gpu.SliverData(gpu.Symbols(bytes(primary[i]), s), i, "primary"))
        slivers.append(gpu.SliverData(gpu.Symbols(bytes(secondary[i]), s), i, "secondary"))
    return meta, slivers


def _corrupt(gpu, slivers, picks):
    out = list(slivers)
    for i in picks:
        d = bytearray(out[i].symbols.data)
        d[len(d) // 2] ^= 0x10
        out[i] = gpu.SliverData(gpu.Symbols(bytes(d), out[i].symbol_size), out[i].index,
                                out[i].axis)
    return out


def _from_scenario(gpu, sc):
    return _blob_slivers(gpu, sc.geo.n, sc.hashes, len(sc.blob), sc.primary, sc.secondary,
                         sc.params.symbol_size)


def _from_engine(gpu, cfg, blob):
    pairs, meta = cfg.encode_with_metadata(blob)
    slivers = [sl for p in pairs for sl in (p.primary, p.secondary)]
    return meta.metadata, slivers


@pytest.mark.parametrize("n", [10, 13])
def test_verify_slivers_of_blobs(gpu, n):
    cfg = gpu.ReedSolomonEncodingConfig(n)
    g3 = corruption.scenario("G3")
    if n == 10:
        blobs = [_from_scenario(gpu, corruption.scenario("G1")), _from_engine(gpu, cfg, g3.blob),
                 _from_scenario(gpu, corruption.scenario("G0_1"))]
    else:
        blob2 = np.random.default_rng(5).integers(0, 256, 700, dtype=np.uint8).tobytes()
        blobs = [_from_scenario(gpu, g3), _from_engine(gpu, cfg, blob2)]
    sizes = {sl[0].symbol_size for _, sl in blobs}
    assert len(sizes) == len(blobs)                       # a symbol size per blob
    blobs = [(meta, _corrupt(gpu, sl, picks)) for (meta, sl), picks in
             zip(blobs, ([0, 7], [3, 2 * n - 1], [1]))]
    got = gpu.verify_slivers_of_blobs(cfg, blobs)
    for b, (meta, slivers) in enumerate(blobs):
        want = gpu.verify_slivers(cfg, meta, slivers)
        assert got[b] == want, b
        assert want.count(False) == (2 if b < 2 else 1)
    assert gpu.verify_slivers_of_blobs(cfg, []) == []
    # the size rules of verify_slivers, per blob
    meta, slivers = blobs[0]
    other = blobs[1][1][0]
    with pytest.raises(ValueError, match="SliverSizeMismatch"):
        gpu.verify_slivers_of_blobs(cfg, [(meta, [other])])
    with pytest.raises(ValueError, match="IndexTooLarge"):
        gpu.verify_slivers_of_blobs(
            cfg, [(meta, [gpu.SliverData(slivers[0].symbols, n, "primary")])])
    k = len(slivers[0].symbols.data) // slivers[0].symbol_size
    s = slivers[0].symbol_size
    if (k * s) % (2 * s) == 0:
        wrong = gpu.SliverData(gpu.Symbols(slivers[0].symbols.data, 2 * s), 0, "primary")
        with pytest.raises(ValueError, match="SymbolSizeMismatch"):
            gpu.verify_slivers_of_blobs(cfg, [(meta, [wrong])])
