"""Status contract of the mixed blob encode (include/walrus_rs2.h): per-blob refusals beside good
blobs -- skipped slots keep their sentinel, the others are right --, status_out NULL returning the
first code with nothing written, the whole-call refusals, n_blobs 0, and the host forms
(rs2_encode_blobs_with_metadata, ReedSolomonEncodingConfig.encode_blobs_with_metadata) against
encode_batch_with_metadata on one mixed list."""
import ctypes

import numpy as np
import pytest
import torch

import encode_mixed as M
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 10
OK, TOO_LARGE, INVALID = _lib.RS2_OK, _lib.RS2_E_DATA_TOO_LARGE, _lib.RS2_E_INVALID_ARGUMENT


def _refused_call(gpu, statuses):
    """Good blobs of several sizes with four refused ones between them."""
    kp, ks = M.shape(N)
    items = M.case(N, [2, 6, 66, 130], 1, "interleaved")[:12]
    lay = M.Layout(N, items)
    lens = [x for x, _ in items]
    boff, poff, soff = list(lay.blob_off), list(lay.prim_off), list(lay.sec_off)
    want = [OK] * len(items)
    lens[1] = kp * ks * 0xFFFE + 1       # no symbol size holds it
    want[1] = TOO_LARGE
    boff[4] += 1                          # odd offsets
    poff[6] += 1
    soff[9] += 1
    want[4] = want[6] = want[9] = INVALID
    d_in = torch.tensor(lay.blobs(), device=M.dev())
    full = lambda k: torch.full((k,), M.FILL, dtype=torch.uint8, device=M.dev())  # noqa: E731
    prim, sec = full(lay.prim_bytes), full(lay.sec_bytes)
    hashes, ids = full(len(items) * N * 64), full(len(items) * 32)
    torch.cuda.synchronize()
    rc = gpu.BlobEncoder(N).encode_async(lens, d_in.data_ptr(), boff, prim.data_ptr(), poff,
                                         sec.data_ptr(), soff, hashes.data_ptr(), ids.data_ptr(),
                                         None, statuses)
    torch.cuda.synchronize()
    return M.Out(rc, lay, prim, sec, hashes, ids), want


def test_refused_blobs_are_skipped(gpu):
    before = M.stats()
    out, want = _refused_call(gpu, True)
    assert out.rc == want
    skipped = {i for i, c in enumerate(want) if c != OK}
    M.check(N, out, "refusals beside good blobs", skipped=skipped)
    windows, grouped, single, _, launches = M.moved(before)
    assert grouped + single == len(want) - len(skipped)
    assert launches == windows * M.LAUNCHES  # the good blobs are not neighbours: the scatter runs


def test_null_status_returns_the_first_code(gpu):
    before = M.stats()
    out, want = _refused_call(gpu, False)
    assert out.rc == TOO_LARGE
    assert M.moved(before) == [0, 0, 0, 0, 0]
    for t in (out.primary, out.secondary, out.hashes, out.ids):
        assert bool((t == M.FILL).all()), "a refused call wrote something"


def _raw(handle, m, lens, base, boff, pbase, poff, sbase, soff, hashes, ids, status=None):
    arr = lambda v: None if v is None else (ctypes.c_uint64 * max(len(v), 1))(*v)  # noqa: E731
    return _lib.lib().rs2_blob_encoder_encode_device_async(
        handle, m, arr(lens), base, arr(boff), pbase, arr(poff), sbase, arr(soff), hashes, ids,
        status, None)


def test_whole_call_refusals_and_empty_call(gpu):
    items = M.case(N, [4, 6], 1)[:3]
    lay = M.Layout(N, items)
    lens = [x for x, _ in items]
    d_in = torch.tensor(lay.blobs(), device=M.dev())
    full = lambda k: torch.full((k + 32,), M.FILL, dtype=torch.uint8, device=M.dev())  # noqa: E731
    prim, sec, hashes, ids = full(lay.prim_bytes), full(lay.sec_bytes), full(3 * N * 64), full(96)
    enc = gpu.BlobEncoder(N)
    h = enc.handle
    good = dict(lens=lens, base=d_in.data_ptr(), boff=lay.blob_off, pbase=prim.data_ptr(),
                poff=lay.prim_off, sbase=sec.data_ptr(), soff=lay.sec_off,
                hashes=hashes.data_ptr(), ids=ids.data_ptr())

    def call(handle=h, m=3, **kw):
        return _raw(handle, m, **{**good, **kw})

    before = M.stats()
    torch.cuda.synchronize()
    assert call(handle=None) == INVALID
    for name in ("lens", "base", "boff", "hashes", "ids", "poff", "soff"):
        assert call(**{name: None}) == INVALID, name
    assert call(pbase=None) == INVALID and call(sbase=None) == INVALID  # one without the other
    assert call(base=good["base"] + 1) == INVALID
    assert call(pbase=good["pbase"] + 1) == INVALID
    assert call(sbase=good["sbase"] + 1) == INVALID
    assert call(hashes=good["hashes"] + 8) == INVALID
    assert call(ids=good["ids"] + 2) == INVALID
    big = [4] * 65536
    assert call(m=65536, lens=big, boff=big, poff=big, soff=big) == INVALID
    # n_blobs 0: RS2_OK with nothing enqueued, whatever the arrays
    assert call(m=0) == OK
    assert call(m=0, lens=None, base=None, boff=None, hashes=None, ids=None) == OK
    status = (ctypes.c_int * 3)(7, 7, 7)
    assert call(m=0, status=status) == OK and list(status) == [7, 7, 7]
    torch.cuda.synchronize()
    assert M.moved(before) == [0, 0, 0, 0, 0]
    for t in (prim, sec, hashes, ids):
        assert bool((t == M.FILL).all())
    # and the same arguments, unchanged, run
    assert call() == OK
    torch.cuda.synchronize()
    out = M.Out(OK, lay, prim[:lay.prim_bytes], sec[:lay.sec_bytes], hashes[:3 * N * 64], ids[:96])
    M.check(N, out, "the good call")


MIXED = [(10, [1, 56, 57, 111, 112, 113, 1847, 3700, 0]), (100, [5000, 2 * 34 * 67, 30001, 9112, 150000])]


@pytest.mark.parametrize("n,lens", MIXED)
def test_host_forms_match_the_batch_call(gpu, n, lens):
    rng = np.random.default_rng(n)
    blobs = [rng.integers(0, 256, x, dtype=np.uint8).tobytes() for x in lens]
    cfg = gpu.ReedSolomonEncodingConfig(n)
    want = cfg.encode_batch_with_metadata(blobs)
    before = M.stats()
    got = cfg.encode_blobs_with_metadata(blobs)
    windows, grouped, single, _, _ = M.moved(before)
    sizes = [M.sym(n, x) for x in lens]
    # the s = 2 blobs go to the per-size batch call, the others through one mixed call
    assert (windows, grouped, single) == (1, sum(s >= 4 for s in sizes), 0)
    assert len(got) == len(want) == len(blobs)
    for i, ((gp, gm), (wp, wm)) in enumerate(zip(got, want)):
        assert bytes(gm.blob_id) == bytes(wm.blob_id), i
        assert gm.metadata.hashes == wm.metadata.hashes, i
        assert gm.metadata.unencoded_length == wm.metadata.unencoded_length == lens[i]
        for k, (a, b) in enumerate(zip(gp, wp)):
            assert a.primary.symbols.data == b.primary.symbols.data, (i, k)
            assert a.secondary.symbols.data == b.secondary.symbols.data, (i, k)
            assert (a.primary.index, a.secondary.index) == (b.primary.index, b.secondary.index)
            assert a.primary.symbols.symbol_size == sizes[i]


def test_host_form_statuses(gpu):
    """rs2_encode_blobs_with_metadata itself: every size through the one call (s = 2 on its
    per-blob path), a NULL blob of non-zero length refused and its slots left alone."""
    n = N
    kp, ks = M.shape(n)
    lens = [57, 0, 300, 20, 1000]
    blobs = [M.blob(n, x, 1) if x else None for x in lens]
    m = len(lens)
    bp = (ctypes.c_void_p * m)(*[None if (b is None or i == 2) else b.ctypes.data
                                 for i, b in enumerate(blobs)])
    cl = (ctypes.c_uint64 * m)(*lens)
    sizes = [M.sym(n, x) for x in lens]
    prim = [np.full((n, ks * s), M.FILL, dtype=np.uint8) for s in sizes]
    sec = [np.full((n, kp * s), M.FILL, dtype=np.uint8) for s in sizes]
    pp = (ctypes.c_void_p * (m * n))(*[prim[b][k].ctypes.data for b in range(m) for k in range(n)])
    sp = (ctypes.c_void_p * (m * n))(*[sec[b][k].ctypes.data for b in range(m) for k in range(n)])
    hashes = np.full(m * n * 64, M.FILL, dtype=np.uint8)
    ids = np.full(m * 32, M.FILL, dtype=np.uint8)
    status = (ctypes.c_int * m)(*([7] * m))
    fn = _lib.lib().rs2_encode_blobs_with_metadata
    assert fn(n, m, bp, cl, pp, sp, hashes.ctypes.data, ids.ctypes.data, None) == INVALID
    assert (hashes == M.FILL).all() and (ids == M.FILL).all()
    assert fn(n, m, bp, cl, pp, sp, hashes.ctypes.data, ids.ctypes.data, status) == OK
    assert list(status) == [OK, OK, INVALID, OK, OK]
    cfg = gpu.ReedSolomonEncodingConfig(n)
    for b, x in enumerate(lens):
        h, i = hashes[b * n * 64:(b + 1) * n * 64], ids[b * 32:(b + 1) * 32]
        if b == 2:
            for a in (prim[b], sec[b], h, i):
                assert (a == M.FILL).all(), "a slot of the refused blob was written"
            continue
        pairs, meta = cfg.encode_with_metadata(blobs[b].tobytes() if x else b"")
        assert bytes(i) == bytes(meta.blob_id), b
        assert h.tobytes() == b"".join(p + s for p, s in meta.metadata.hashes), b
        for k in range(n):
            assert prim[b][k].tobytes() == pairs[k].primary.symbols.data, (b, k)
            assert sec[b][n - 1 - k].tobytes() == pairs[k].secondary.symbols.data, (b, k)
    assert fn(n, 0, None, None, None, None, None, None, None) == OK
    assert fn(n, 65536, bp, cl, pp, sp, None, None, None) == INVALID
    assert fn(n, m, None, cl, pp, sp, None, None, None) == INVALID
