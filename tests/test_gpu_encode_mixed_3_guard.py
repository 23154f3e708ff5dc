"""Containment of rs2_blob_encoder_encode_device_async (tests/guarded.py): blobs, slivers, hashes
and ids live in guard-band buffers, the 2-byte-aligned ones at every payload residue of
guarded.DELTAS.  The blobs are packed back to back, so a read past a blob's end reads the next blob
(or the guard); the slivers have gaps between them that must keep the pattern.  The same call runs
with two fills of the input buffer -- what lies between and around the blobs differs, the outputs
may not -- and then with the blobs in reverse order, so every blob has other neighbours: each
blob's outputs must be the same bytes again."""
import pytest
import torch

import encode_mixed as M
from guarded import DELTAS, Guarded

pytestmark = pytest.mark.gpu

SIZES = {10: M.SIZES, 100: [2, 6, 66, 130, 258]}


def _run(enc, n, items, delta, fill, meta_only=False):
    lay = M.Layout(n, items, gap=6)
    m = len(items)
    g_in = Guarded(lay.blob_bytes, delta, M.dev(), fill)
    for (x, seed), o in zip(items, lay.blob_off):
        g_in.set(M.blob(n, x, seed).tobytes(), o)
    before = g_in.buf.clone()
    g_p = Guarded(lay.prim_bytes, delta, M.dev(), 11)
    g_s = Guarded(lay.sec_bytes, (delta + 6) % 16, M.dev(), 23)
    g_h = Guarded(m * n * 64, 0, M.dev(), 37)
    g_i = Guarded(m * 32, 0, M.dev(), 41)
    torch.cuda.synchronize()
    rc = enc.encode_async([x for x, _ in items], g_in.ptr, lay.blob_off,
                          0 if meta_only else g_p.ptr, None if meta_only else lay.prim_off,
                          0 if meta_only else g_s.ptr, None if meta_only else lay.sec_off,
                          g_h.ptr, g_i.ptr)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(g_in.buf, before), "the input buffer was written"
    g_p.assert_guards_intact([] if meta_only else list(zip(lay.prim_off, lay.prim_len)), "d_primary")
    g_s.assert_guards_intact([] if meta_only else list(zip(lay.sec_off, lay.sec_len)), "d_secondary")
    g_h.assert_guards_intact(None, "d_hashes")
    g_i.assert_guards_intact(None, "d_blob_ids")
    out = {}
    for i, (x, seed) in enumerate(items):
        ref = M.reference(n, x, seed)
        got = {"hashes": g_h.payload[i * n * 64:(i + 1) * n * 64],
               "id": g_i.payload[i * 32:(i + 1) * 32]}
        want = {"hashes": ref.hashes, "id": ref.blob_id}
        if not meta_only:
            got["primary"] = g_p.payload[lay.prim_off[i]:lay.prim_off[i] + lay.prim_len[i]]
            got["secondary"] = g_s.payload[lay.sec_off[i]:lay.sec_off[i] + lay.sec_len[i]]
            want["primary"], want["secondary"] = ref.primary, ref.secondary
        for k in got:
            assert torch.equal(got[k], want[k]), \
                f"n={n} delta={delta} fill={fill}: {k} of blob {i} (length {x}) differs"
        out[(x, seed)] = {k: v.clone() for k, v in got.items()}
    return out


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("n", [10, 100])
def test_guards_fills_and_neighbours(gpu, n, delta):
    enc = gpu.BlobEncoder(n)
    items = M.case(n, SIZES[n], 1, "interleaved")
    runs = [_run(enc, n, items, delta, 0), _run(enc, n, items, delta, 77),
            _run(enc, n, items[::-1], delta, 5)]
    for other in runs[1:]:
        for key, got in runs[0].items():
            for k, v in got.items():
                assert torch.equal(v, other[key][k]), (key, k)


@pytest.mark.parametrize("n", [10, 100])
def test_metadata_only_writes_no_sliver(gpu, n):
    enc = gpu.BlobEncoder(n)
    items = M.case(n, SIZES[n], 1, "interleaved")
    a = _run(enc, n, items, 2, 0, meta_only=True)
    b = _run(enc, n, items[::-1], 14, 99, meta_only=True)
    for key, got in a.items():
        for k, v in got.items():
            assert torch.equal(v, b[key][k]), (key, k)
