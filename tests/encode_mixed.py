"""Helpers of the mixed blob encode tests (tests/test_gpu_encode_mixed_*.py) -- TEST ONLY, a plain
module.  A case is a list of items (blob length, seed): blob bytes are seeded random, their
reference slivers, pair hashes and id come from oracle.encode_with_metadata below n = 1000 and from
the per-blob device encode (rs2_encode_device_async, which the goldens pin) at n = 1000 and above --
once per (n, length, seed), shared and left unchanged.  `run` issues one
rs2_blob_encoder_encode_device_async call on torch buffers and returns what it wrote."""
import ctypes

import numpy as np
import torch

import rs2_oracle as O
from walrus_amd import _lib

SIZES = [2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258]
SIZES_1000 = [2, 20, 66, 130]
FILL = 0xEE            # outputs hold this before a call
POOL = 2               # distinct blobs per (n, length): member j of a kind is seed j % POOL
LAUNCHES = _lib.RS2_ENCODE_MIXED_WINDOW_LAUNCHES
ORDERS = ("interleaved", "sorted", "reverse")


def sizes_of(n):
    return SIZES_1000 if n >= 1000 else SIZES


def shape(n):
    return O.source_symbols_for_n_shards(n)


def sym(n, length):
    kp, ks = shape(n)
    return O.compute_symbol_size(length, kp * ks)


def mid_len(n, s):
    """A length of symbol size s that ends inside a row and inside a symbol."""
    kp, ks = shape(n)
    lo, hi = (s - 2) * kp * ks + 1, s * kp * ks
    length = lo + (hi - lo) // 2
    while length % s == 0 or (length // s) % ks == 0:
        length += 1
    return length


def lengths(n, s):
    """The lengths of symbol size s: exact, an odd tail, nearly all of the last symbols padding,
    one that ends mid-row and mid-symbol; at n = 10 also length 1."""
    kp, ks = shape(n)
    full = s * kp * ks
    out = [full, full - 1, (s - 2) * kp * ks + 1, mid_len(n, s)]
    if n == 10 and s == 2:
        out.append(1)
    assert all(sym(n, x) == s for x in out), (n, s, out)
    return out


def scratch(n, s, meta_only=False):
    """Window scratch of one blob (include/walrus_rs2.h)."""
    kp, ks = shape(n)
    return (n - kp) * (n - ks) * s + 32 * n * n + (n * (kp + ks) * s if meta_only else 0)


def eligible(n, s):
    return s >= 4 and n <= 4096


def case(n, sizes, per, order="interleaved"):
    """Items (length, seed) over sizes x their lengths, `per` blobs per kind."""
    kinds = [x for s in sizes for x in lengths(n, s)]
    if order == "interleaved":
        items = [(x, j) for j in range(per) for x in kinds]
    else:
        items = [(x, j) for x in kinds for j in range(per)]
        if order == "reverse":
            items.reverse()
    return [(x, j % POOL) for x, j in items]


def dev():
    return torch.device("cuda", 0)


_BLOBS, _REFS = {}, {}


def blob(n, length, seed=0):
    key = (n, length, seed)
    if key not in _BLOBS:
        rng = np.random.default_rng([n, length, seed, 4321])
        a = rng.integers(1, 256, length, dtype=np.uint8)  # no zero byte: padding is told apart
        a.setflags(write=False)
        _BLOBS[key] = a
    return _BLOBS[key]


class Ref:
    """Reference outputs of one blob as device tensors: primary (n*K_s*s), secondary (n*K_p*s),
    hashes (64 n), blob id (32)."""

    def __init__(self, primary, secondary, hashes, blob_id):
        self.primary, self.secondary, self.hashes, self.blob_id = primary, secondary, hashes, blob_id


def _oracle_ref(n, length, seed):
    ref = O.encode_with_metadata(blob(n, length, seed).tobytes(), n)
    hashes = b"".join(p + s for p, s in ref.pair_hashes)
    t = lambda a: torch.tensor(np.frombuffer(bytes(a), dtype=np.uint8).copy(), device=dev())  # noqa: E731
    return Ref(t(ref.primary.tobytes()), t(ref.secondary.tobytes()), t(hashes), t(ref.blob_id))


def _device_ref(n, length, seed):
    """The existing per-blob device encode (its outputs are pinned by the goldens and the oracle
    tests of the single-blob path)."""
    import walrus_amd as W
    kp, ks = shape(n)
    s = sym(n, length)
    plan = W.DevicePlan(n, length)
    d_blob = torch.tensor(blob(n, length, seed), device=dev())
    prim = torch.zeros(n * ks * s, dtype=torch.uint8, device=dev())
    sec = torch.zeros(n * kp * s, dtype=torch.uint8, device=dev())
    hashes = torch.zeros(n * 64, dtype=torch.uint8, device=dev())
    bid = torch.zeros(32, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    plan.encode_async(d_blob.data_ptr(), prim.data_ptr(), sec.data_ptr(), hashes.data_ptr(),
                      bid.data_ptr())
    plan.sync()
    torch.cuda.synchronize()
    return Ref(prim, sec, hashes, bid)


def reference(n, length, seed=0):
    key = (n, length, seed)
    if key not in _REFS:
        _REFS[key] = (_device_ref if n >= 1000 else _oracle_ref)(n, length, seed)
    return _REFS[key]


class Layout:
    """Where the items' blobs and slivers lie: blobs packed back to back at 2-byte steps (a read
    past a blob's end reads the next blob), slivers with `gap` bytes between neighbours."""

    def __init__(self, n, items, gap=6):
        kp, ks = shape(n)
        self.n, self.items = n, list(items)
        self.sizes = [sym(n, x) for x, _ in items]
        self.blob_off, self.prim_off, self.sec_off = [], [], []
        at = pat = sat = 0
        for (x, _), s in zip(items, self.sizes):
            self.blob_off.append(at)
            self.prim_off.append(pat)
            self.sec_off.append(sat)
            at += (x + 1) // 2 * 2
            pat += n * ks * s + gap
            sat += n * kp * s + gap
        self.blob_bytes, self.prim_bytes, self.sec_bytes = max(at, 2), max(pat, 2), max(sat, 2)
        self.prim_len = [n * ks * s for s in self.sizes]
        self.sec_len = [n * kp * s for s in self.sizes]

    def blobs(self, pad=0x5A):
        buf = np.full(self.blob_bytes, pad, dtype=np.uint8)
        for (x, seed), o in zip(self.items, self.blob_off):
            buf[o:o + x] = blob(self.n, x, seed)
        return buf


def stats():
    out = (ctypes.c_uint64 * 5)()
    assert _lib.lib().rs2_encode_mixed_stats(out) == 0
    return [int(x) for x in out]


def moved(before):
    return [a - b for a, b in zip(stats(), before)]


def set_budget(nbytes):
    assert _lib.lib().rs2_set_encode_mixed_budget(int(nbytes)) == 0


class Out:
    def __init__(self, rc, lay, primary, secondary, hashes, ids):
        self.rc, self.lay = rc, lay
        self.primary, self.secondary, self.hashes, self.ids = primary, secondary, hashes, ids


def run(encoder, n, items, meta_only=False, statuses=False, stream=None, gap=6, lay=None):
    """One call over `items`.  Returns an Out after a device synchronize; every output starts as
    FILL."""
    lay = lay or Layout(n, items, gap)
    m = len(items)
    d_in = torch.tensor(lay.blobs(), device=dev())
    full = lambda k: torch.full((max(k, 16),), FILL, dtype=torch.uint8, device=dev())  # noqa: E731
    prim, sec = (None, None) if meta_only else (full(lay.prim_bytes), full(lay.sec_bytes))
    hashes, ids = full(m * n * 64), full(m * 32)
    torch.cuda.synchronize()
    rc = encoder.encode_async(
        [x for x, _ in items], d_in.data_ptr(), lay.blob_off,
        0 if meta_only else prim.data_ptr(), None if meta_only else lay.prim_off,
        0 if meta_only else sec.data_ptr(), None if meta_only else lay.sec_off,
        hashes.data_ptr(), ids.data_ptr(), stream, statuses)
    torch.cuda.synchronize()
    return Out(rc, lay, prim, sec, hashes, ids)


def check(n, out, what="", skipped=()):
    """Every accepted blob's outputs equal its reference; everything else still holds FILL."""
    lay = out.lay
    bad = []
    for i, (x, seed) in enumerate(lay.items):
        h = out.hashes[i * n * 64:(i + 1) * n * 64]
        b = out.ids[i * 32:(i + 1) * 32]
        p = None if out.primary is None else out.primary[lay.prim_off[i]:lay.prim_off[i] + lay.prim_len[i]]
        s = None if out.secondary is None else out.secondary[lay.sec_off[i]:lay.sec_off[i] + lay.sec_len[i]]
        if i in skipped:
            for name, t in (("hashes", h), ("id", b), ("primary", p), ("secondary", s)):
                if t is not None and not bool((t == FILL).all()):
                    bad.append((i, x, name + " of a skipped blob written"))
            continue
        ref = reference(n, x, seed)
        for name, t, r in (("primary", p, ref.primary), ("secondary", s, ref.secondary),
                           ("hashes", h, ref.hashes), ("id", b, ref.blob_id)):
            if t is not None and not torch.equal(t, r):
                d = torch.nonzero(t != r).reshape(-1)
                bad.append((i, x, f"{name}: {d.numel()} of {t.numel()} bytes differ, first at {int(d[0])}"))
    assert not bad, f"{what}: {len(bad)} findings, the first {bad[:4]}"
    # the gaps between slivers and the slack behind the last one are not written
    for buf, offs, lens in ((out.primary, lay.prim_off, lay.prim_len),
                            (out.secondary, lay.sec_off, lay.sec_len)):
        if buf is None:
            continue
        at = 0
        for o, ln in sorted((o, ln) for i, (o, ln) in enumerate(zip(offs, lens)) if i not in skipped):
            assert bool((buf[at:o] == FILL).all()), f"{what}: bytes before offset {o} were written"
            at = o + ln
        assert bool((buf[at:] == FILL).all()), f"{what}: bytes behind the last sliver were written"
