"""Batched blob decode (rs2_decode_batch_device_async / rs2_decode_batch / decode_batch): many
blobs of one symbol size, an erasure pattern per blob, one launch per chunk.  The source blob is
the reference everywhere; slivers come from the oracle at n = 10 and 13 and from the engine's
own (oracle-checked) encode above.  rs2_decode_batch_stats deltas pin which path each blob took."""
import ctypes

import numpy as np
import pytest
import torch

import rs2_oracle as O
from guarded import Guarded

pytestmark = pytest.mark.gpu

FILL = 7
OK, E_NOT_ENOUGH, E_UNSUCCESSFUL, E_INVALID = 0, -5, -6, -8


def _stats():
    from walrus_amd.encoding import decode_batch_stats
    s = decode_batch_stats()
    return np.array([s["launches"], s["batched"], s["single"]], dtype=np.int64)


def _lens_for(n, s, count, rng):
    """`count` distinct blob lengths whose symbol size at n shards is s (the largest included)."""
    kp, ks = O.source_symbols_for_n_shards(n)
    lo, hi = (s - 2) * kp * ks + 1, s * kp * ks
    lens = {hi}
    while len(lens) < count:
        lens.add(int(rng.integers(lo, hi + 1)))
    lens = sorted(lens, reverse=True)
    for ln in lens:
        assert O.compute_symbol_size(ln, kp * ks) == s
    return lens


class Encoded:
    """B blobs of one symbol size with their slivers on the device: prim[b] = n primary slivers
    back to back, sec[b] likewise."""

    def __init__(self, W, n, blobs, oracle):
        self.n, self.blobs, self.B = n, blobs, len(blobs)
        self.lens = [len(b) for b in blobs]
        self.plan = W.DevicePlan(n, max(self.lens))
        info = self.plan.info
        self.kp, self.ks, self.s = info.n_primary, info.n_secondary, info.symbol_size
        self.pl, self.sl = info.primary_sliver_len, info.secondary_sliver_len
        dev = torch.device("cuda", 0)
        B = self.B
        if oracle:
            prim = np.zeros((B, n * self.pl), dtype=np.uint8)
            sec = np.zeros((B, n * self.sl), dtype=np.uint8)
            for b, blob in enumerate(blobs):
                p = O.Rs2Params.for_blob(n, len(blob))
                assert p.symbol_size == self.s
                x = O.expanded_matrix(blob.tobytes(), p)
                prim[b] = x[:, :self.ks].reshape(-1)
                sec[b] = np.ascontiguousarray(x[:self.kp].transpose(1, 0, 2)).reshape(-1)
            self.prim = torch.from_numpy(prim).to(dev)
            self.sec = torch.from_numpy(sec).to(dev)
        else:
            stride = (max(self.lens) + 255) // 256 * 256
            d_blobs = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
            for b, blob in enumerate(blobs):
                d_blobs[b * stride:b * stride + len(blob)] = torch.from_numpy(blob).to(dev)
            self.prim = torch.empty((B, n * self.pl), dtype=torch.uint8, device=dev)
            self.sec = torch.empty((B, n * self.sl), dtype=torch.uint8, device=dev)
            hashes = torch.empty(B * n * 64, dtype=torch.uint8, device=dev)
            ids = torch.empty(B * 32, dtype=torch.uint8, device=dev)
            self.plan.encode_batch_async(B, d_blobs.data_ptr(), stride, self.lens,
                                         self.prim.data_ptr(), n * self.pl, self.sec.data_ptr(),
                                         n * self.sl, hashes.data_ptr(), ids.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
        self.dev_blobs = [torch.from_numpy(b).to(dev) for b in blobs]

    def axis(self, axis):
        """(slivers tensor, sliver length, K) of an axis."""
        return ((self.prim, self.pl, self.kp) if axis == "primary" else (self.sec, self.sl, self.ks))

    def decode(self, axis, subsets, which=None, stride=None, statuses=False, lens=None, out=None):
        """Batch-decode blobs `which` (default all) from `subsets` into a 7-filled buffer."""
        which = list(range(self.B)) if which is None else which
        sl, L, _ = self.axis(axis)
        stride = stride or (max(self.lens) + 37) // 2 * 2
        if out is None:
            out = torch.full((len(which) * stride + 64,), FILL, dtype=torch.uint8, device=sl.device)
        items = [(sel, [(b * self.n + i) * L for i in sel]) for b, sel in zip(which, subsets)]
        st = torch.cuda.current_stream(sl.device).cuda_stream
        codes = self.plan.decode_batch_async(
            axis, items, sl.data_ptr(), out.data_ptr(), stride,
            lens if lens is not None else [self.lens[b] for b in which], st, statuses)
        return out, stride, codes

    def check(self, out, stride, which=None, skipped=()):
        """Blobs equal their sources; the padding and everything at or past a length is FILL."""
        torch.cuda.synchronize()
        which = list(range(self.B)) if which is None else which
        for k, b in enumerate(which):
            got = out[k * stride:(k + 1) * stride]
            ln = 0 if k in skipped else self.lens[b]
            if ln:
                assert torch.equal(got[:ln], self.dev_blobs[b]), f"blob {b} differs"
            assert bool((got[ln:] == FILL).all()), f"blob {b}: bytes at or past its length written"
        assert bool((out[len(which) * stride:] == FILL).all())


def _subsets(n, K, B, rng):
    """all-repair (topped up with originals when R < K), all-systematic, one erasure, then
    random K-subsets in random order -- a different one per blob."""
    gone = int(rng.integers(K))
    subs = [list(range(n - 1, -1, -1))[:K], list(range(K)),
            [i for i in range(K) if i != gone] + [K + int(rng.integers(n - K))]]
    while len(subs) < B:
        subs.append([int(i) for i in rng.permutation(n)[:K]])
    return subs[:B]


def _random_blobs(lens, rng):
    return [rng.integers(0, 256, ln, dtype=np.uint8) for ln in lens]


# ---- 1. small shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("n,s", [(10, 6), (10, 40), (13, 6), (13, 40)])
def test_small_shapes_device_and_host_forms(gpu, n, s):
    from walrus_amd import _lib
    rng = np.random.default_rng(n * 100 + s)
    B = 6
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, s, B, rng), rng), oracle=True)
    assert enc.s == s
    for axis in ("primary", "secondary"):
        sl, L, K = enc.axis(axis)
        subs = _subsets(n, K, B, rng)
        before = _stats()
        out, stride, _ = enc.decode(axis, subs)
        enc.check(out, stride)
        # the all-systematic blob is a copy (per-blob path), the others share one launch
        assert (_stats() - before).tolist() == [1, B - 1, 1]
        # host form: a repeated sliver, a wrong-length one and a surplus one in every list
        host = sl.cpu().numpy()
        idx, ptrs, lens, keep, counts = [], [], [], [], []
        for b, sel in enumerate(subs):
            spare = next(i for i in range(n) if i not in sel)
            rows = [(sel[0], L), (spare, L - 2)] + [(i, L) for i in sel] + [(spare, L)]
            for i, ln in rows:
                a = np.ascontiguousarray(host[b, i * L:i * L + ln])
                keep.append(a)
                idx.append(i)
                ptrs.append(a.ctypes.data)
                lens.append(ln)
            counts.append(len(rows))
        m = len(idx)
        outs = [np.full(enc.lens[b] + 8, FILL, dtype=np.uint8) for b in range(B)]
        rc = _lib.lib().rs2_decode_batch(
            enc.plan.handle, 0 if axis == "primary" else 1, B,
            (ctypes.c_uint64 * B)(*enc.lens), (ctypes.c_uint32 * B)(*counts),
            (ctypes.c_uint16 * m)(*idx), (ctypes.c_void_p * m)(*ptrs), (ctypes.c_uint64 * m)(*lens),
            None, (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs]), None)
        assert rc == OK, _lib.last_error()
        for b in range(B):
            assert np.array_equal(outs[b][:enc.lens[b]], enc.blobs[b]), (axis, b)
            assert (outs[b][enc.lens[b]:] == FILL).all()


# ---- 2. the C3 shape (shared with 4 and 7) --------------------------------------------------
@pytest.fixture(scope="module")
def c3(gpu):
    rng = np.random.default_rng(1000)
    lens = [4 * (1 << 20) + int(d) for d in rng.integers(-60_000, 60_000, 12)]
    enc = Encoded(gpu, 1000, _random_blobs(lens, rng), oracle=False)
    assert enc.s == 20
    return enc


@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_c3_twelve_blobs_one_launch(c3, axis):
    rng = np.random.default_rng(len(axis))
    K = c3.axis(axis)[2]
    subs = [[int(i) for i in rng.permutation(1000)[:K]] for _ in range(c3.B)]
    before = _stats()
    out, stride, _ = c3.decode(axis, subs, stride=(max(c3.lens) + 4099) // 2 * 2)
    c3.check(out, stride)
    assert (_stats() - before).tolist() == [1, 12, 0]


# ---- 3. lane classes, n_out > 1 -------------------------------------------------------------
@pytest.mark.parametrize("s", [6, 22, 66, 130])
def test_lane_classes_both_axes(gpu, s):
    n, B = 100, 6
    rng = np.random.default_rng(s)
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, s, B, rng), rng), oracle=False)
    assert enc.s == s
    for axis in ("primary", "secondary"):
        K = enc.axis(axis)[2]
        subs = [[int(i) for i in rng.permutation(n)[:K]] for _ in range(B)]
        subs[0] = list(range(n - 1, -1, -1))[:K]  # every output block of the axis
        before = _stats()
        out, stride, _ = enc.decode(axis, subs)
        enc.check(out, stride)
        assert (_stats() - before).tolist() == [1, B, 0]


# ---- 4. block limits ------------------------------------------------------------------------
@pytest.mark.parametrize("limit,batched", [(256, True), (128, False)])
def test_block_limits_at_n1000(c3, limit, batched):
    from walrus_amd import _lib
    rng = np.random.default_rng(limit)
    which = [0, 5, 11]
    try:
        assert _lib.lib().rs2_set_block_limit(limit) == 0
        for axis in ("primary", "secondary"):
            K = c3.axis(axis)[2]
            subs = [[int(i) for i in rng.permutation(1000)[:K]] for _ in which]
            before = _stats()
            out, stride, _ = c3.decode(axis, subs, which=which)
            c3.check(out, stride, which=which)
            assert (_stats() - before).tolist() == ([1, 3, 0] if batched else [0, 0, 3])
    finally:
        assert _lib.lib().rs2_set_block_limit(512) == 0


# ---- 5. fallbacks ---------------------------------------------------------------------------
def test_fallback_many_blocks_n4500(gpu):
    n, B = 4500, 3
    rng = np.random.default_rng(4500)
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, 4, B, rng), rng), oracle=False)
    K = enc.kp
    subs = [[int(i) for i in rng.permutation(n)[:K]] for _ in range(B)]
    before = _stats()
    out, stride, _ = enc.decode("primary", subs)
    enc.check(out, stride)
    assert (_stats() - before).tolist() == [0, 0, B]


def test_fallback_two_byte_symbols_and_mixed_call(gpu):
    n = 10
    rng = np.random.default_rng(5)
    tiny = Encoded(gpu, n, _random_blobs(_lens_for(n, 2, 4, rng), rng), oracle=True)
    subs = [[int(i) for i in rng.permutation(n)[:tiny.kp]] for _ in range(4)]
    before = _stats()
    out, stride, _ = tiny.decode("primary", subs)
    tiny.check(out, stride)
    assert (_stats() - before).tolist() == [0, 0, 4]
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, 6, 4, rng), rng), oracle=True)
    K = enc.ks
    subs = [list(range(K)), [int(i) for i in rng.permutation(n)[:K]], list(range(K))[::-1],
            list(range(n - K, n))]
    before = _stats()
    out, stride, _ = enc.decode("secondary", subs)
    enc.check(out, stride)
    assert (_stats() - before).tolist() == [1, 2, 2]


# ---- 6. more than one chunk -----------------------------------------------------------------
def test_more_than_one_chunk(gpu):
    n, s, distinct, B = 10, 4, 20, 700
    rng = np.random.default_rng(700)
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, s, distinct, rng), rng), oracle=True)
    assert enc.s == s
    # 700 decodes, each with its own subset and output, over the 20 encoded blobs
    which = [k % distinct for k in range(B)]
    subs = []
    while len(subs) < B:
        sel = [int(i) for i in rng.permutation(n)[:enc.kp]]
        if any(i >= enc.kp for i in sel):  # something erased: a batch job
            subs.append(sel)
    before = _stats()
    out, stride, _ = enc.decode("primary", subs, which=which)
    enc.check(out, stride, which=which)
    d = (_stats() - before).tolist()
    assert d[0] >= 2 and d[1:] == [B, 0]


# ---- 7. slot reuse --------------------------------------------------------------------------
def test_back_to_back_calls_keep_their_arrays(c3):
    rng = np.random.default_rng(77)
    calls = []
    for which in ([0, 1, 2], [3, 4, 5], [6, 7, 8]):  # three calls, two slots, no sync between
        subs = [[int(i) for i in rng.permutation(1000)[:c3.kp]] for _ in which]
        calls.append((which,) + c3.decode("primary", subs, which=which)[:2])
    for which, out, stride in calls:
        c3.check(out, stride, which=which)


# ---- 8. errors ------------------------------------------------------------------------------
def test_errors_per_blob_and_whole_call(gpu):
    from walrus_amd import _lib
    n, B = 13, 4
    rng = np.random.default_rng(8)
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, 6, B, rng), rng), oracle=True)
    sl, L, K = enc.axis("primary")
    good = [[int(i) for i in rng.permutation(n)[:K]] for _ in range(B)]
    other_len = _lens_for(n, 8, 1, rng)[0]
    lib, h = _lib.lib(), enc.plan.handle
    st = torch.cuda.current_stream(sl.device).cuda_stream
    stride = max(enc.lens) + 10

    def call(subs, lens=None, offsets=None, out_stride=stride, status=False, n_blobs=B):
        lens = enc.lens if lens is None else lens
        offs = offsets or [[(b * n + i) * L for i in sel] for b, sel in enumerate(subs)]
        flat_i = [i for sel in subs for i in sel]
        flat_o = [o for of in offs for o in of]
        m = max(len(flat_i), 1)
        out = torch.full((B * stride + 64,), FILL, dtype=torch.uint8, device=sl.device)
        codes = (ctypes.c_int * B)(*([99] * B)) if status else None
        rc = lib.rs2_decode_batch_device_async(
            h, 0, n_blobs, (ctypes.c_uint64 * B)(*lens),
            (ctypes.c_uint32 * B)(*[len(sel) for sel in subs]), (ctypes.c_uint16 * m)(*flat_i),
            sl.data_ptr(), (ctypes.c_uint64 * m)(*flat_o), out.data_ptr(), out_stride, codes, st)
        torch.cuda.synchronize()
        return rc, out, (list(codes) if status else None)

    few = [good[0], good[1][:K - 1], good[2], good[3]]
    big = [good[0], good[1], [n] + good[2][1:], good[3]]
    odd_off = [[(b * n + i) * L + (1 if b == 3 else 0) for i in sel] for b, sel in enumerate(good)]
    wrong_len = [enc.lens[0], other_len, enc.lens[2], enc.lens[3]]
    # status_out NULL: the first failing blob's code, nothing enqueued
    for kwargs, want in ((dict(subs=few), E_UNSUCCESSFUL), (dict(subs=big), E_NOT_ENOUGH),
                         (dict(subs=good, lens=wrong_len), E_INVALID),
                         (dict(subs=good, offsets=odd_off), E_INVALID),
                         (dict(subs=good, out_stride=stride + 1), E_INVALID)):
        rc, out, _ = call(**kwargs)
        assert rc == want, (kwargs.keys(), rc, _lib.last_error())
        assert bool((out == FILL).all())
    # status_out given: codes per blob, the good blobs decoded, the bad ones untouched
    for kwargs, bad, want in ((dict(subs=few), 1, E_UNSUCCESSFUL), (dict(subs=big), 2, E_NOT_ENOUGH),
                              (dict(subs=good, lens=wrong_len), 1, E_INVALID),
                              (dict(subs=good, offsets=odd_off), 3, E_INVALID)):
        rc, out, codes = call(status=True, **kwargs)
        assert rc == OK and codes == [want if b == bad else OK for b in range(B)]
        enc.check(out, stride, skipped=(bad,))
    # an odd stride fails the whole call, whatever status_out is
    rc, out, codes = call(subs=good, out_stride=stride + 1, status=True)
    assert rc == E_INVALID and bool((out == FILL).all())
    # no blobs: nothing to do
    rc, out, _ = call(subs=good, n_blobs=0)
    assert rc == OK and bool((out == FILL).all())


# ---- 9. containment -------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0, 2, 6, 14])
def test_containment_guard_bands(gpu, delta):
    n, B = 13, 4
    rng = np.random.default_rng(9)
    enc = Encoded(gpu, n, _random_blobs(_lens_for(n, 6, B, rng), rng), oracle=True)
    dev = enc.prim.device
    st = torch.cuda.current_stream(dev).cuda_stream
    for axis in ("primary", "secondary"):
        sl, L, K = enc.axis(axis)
        subs = _subsets(n, K, B, rng)
        stride = max(enc.lens) + 6
        items = [(sel, [(b * n + i) * L for i in sel]) for b, sel in enumerate(subs)]
        results = []
        for fill in (0, 91):
            src = Guarded(sl.numel(), delta, dev, fill).set(sl.reshape(-1))
            dst = Guarded(B * stride, delta, dev, 33)
            enc.plan.decode_batch_async(axis, items, src.ptr, dst.ptr, stride, enc.lens, st)
            torch.cuda.synchronize()
            dst.assert_guards_intact([(b * stride, enc.lens[b]) for b in range(B)], "blobs out")
            src.assert_guards_intact(None, "slivers in")
            for b in range(B):
                got = dst.payload[b * stride:b * stride + enc.lens[b]]
                assert torch.equal(got, enc.dev_blobs[b]), (axis, b)
            results.append(dst.payload.clone())
        assert torch.equal(results[0], results[1])  # nothing read from outside the slivers


# ---- 10. Python ------------------------------------------------------------------------------
def test_python_decode_batch_matches_decode(gpu):
    n = 13
    rng = np.random.default_rng(10)
    cfg = gpu.ReedSolomonEncodingConfig(n)
    kp, ks = cfg.n_primary_source_symbols, cfg.n_secondary_source_symbols
    sizes = [0, 70, 333, 71, 2000, 334, 1]
    jobs = []
    for k, size in enumerate(sizes):
        blob = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        pairs, _ = cfg.encode_with_metadata(blob)
        if k % 2:
            sel = [pairs[int(i)].primary for i in rng.permutation(n)[:kp + 1]]
        else:
            sel = [pairs[n - 1 - int(i)].secondary for i in rng.permutation(n)[:ks]]
        jobs.append((blob, size, sel))
    before = _stats()
    got = cfg.decode_batch([(size, sel) for _, size, sel in jobs])
    assert (_stats() - before)[1:].sum() == len(sizes)
    assert got == [blob for blob, _, _ in jobs]
    assert got == [cfg.decode(size, sel) for _, size, sel in jobs]
