"""The plan-level device entry points inside guard bands: encode_async, encode_split_async,
compute_metadata_async, encode_batch_async, decode_async on both axes, and decode_and_verify
with the default and the strict check.

Every buffer has exactly its documented extent (include/walrus_rs2.h; no slack) and lies in
the interior of a tests/guarded.Guarded allocation.  The symbol-carrying buffers (blob,
slivers, decoded blob) are placed at each even residue `delta` mod 16, the digest buffers stay
16-byte aligned.  For every case and placement:

  A  containment   the guards of every output, the stride padding of batch slivers and every
                   byte at or past blob_len of a decoded blob keep their pattern
  B  independence  another fill of the inputs' guards gives bit-identical outputs
  C  correctness   slivers, pair hashes and BlobId equal the C restatement (oracle/rs2_cpu.c
                   through make_fullsize.load_cpu); a decode returns the blob it encoded

The decode is run where its truncation bites: with K = K_p*K_s symbols of s bytes the blob
lengths of symbol size s are L_min = (s-2)K + 1 .. L_max = sK, and the cut falls on L_min, just
past a symbol boundary, a whole symbol short, inside a dword at an odd byte, one byte short and
nowhere; each from all systematic slivers (pure copy-out), from no systematic sliver (every
byte a decode store) and from a random subset (fused copy-out beside stores).

  blob_encoding.rs:277-368 encode_with_metadata      blob_encoding.rs:888-993 decode
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from guarded import DELTAS, Guarded, strided_mask

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_fullsize import load_cpu  # noqa: E402

# n = 1000 reaches the C = 512 kernels and the paired P/Q decode blocks
SHAPES = ([(10, s) for s in (2, 4, 6, 62, 64, 66, 130)] + [(100, s) for s in (2, 6, 66)] +
          [(1000, s) for s in (2, 6, 66)])
LENGTH_KINDS = ("Lmin", "past_symbol", "symbol_short", "odd_in_dword", "one_short", "Lmax")
SUBSETS = ("systematic", "no_systematic", "random")


def deltas_for(n, s):
    return DELTAS if n < 1000 or s == 6 else (0, 2)


def _params(cpu, n, length):
    kp, ks, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    cpu.rs2cpu_params(n, length, ctypes.byref(kp), ctypes.byref(ks), ctypes.byref(s))
    return kp.value, ks.value, s.value


def lengths_for(cpu, n, s):
    """{kind: blob_len}, every one of symbol size s (checked with rs2cpu_params)."""
    kp, ks, _ = _params(cpu, n, 1)
    k = kp * ks
    l_min, l_max = (s - 2) * k + 1, s * k
    # the first length past a symbol boundary above L_min.  A size class spans 2K - 1 lengths, so
    # for s > 2K (n = 10: K = 28, s >= 62) it may hold no symbol boundary at all; those shapes
    # take L_min + 1 in its place (still a cut inside a symbol); nor can such a class cut a
    # whole symbol (L_max - s < L_min), so there the deepest cut it has, L_min, stands in; and
    # where even L_max - s/2 - 1 falls below L_min (n = 10, s = 130) the cut inside a dword is
    # L_max - 3
    past = (l_min // s + 1) * s + 1
    out = {
        "Lmin": l_min,
        "past_symbol": past if past <= l_max else l_min + 1,
        "symbol_short": max(l_max - s, l_min),     # the last symbol wholly cut
        # the cut inside a dword (an odd byte when s/2 is even)
        "odd_in_dword": l_max - s // 2 - 1 if l_max - s // 2 - 1 >= l_min else l_max - 3,
        "one_short": l_max - 1,
        "Lmax": l_max,
    }
    for kind, length in out.items():
        assert max(l_min, 1) <= length <= l_max, (n, s, kind, length)
        assert _params(cpu, n, length) == (kp, ks, s), (n, s, kind, length)
    assert past > l_max or (past % s == 1 and past - s - 1 <= l_min)
    assert (past <= l_max and l_max - s >= l_min) or s > 2 * k - 2
    assert out["one_short"] % 2 == 1
    return out


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


@pytest.mark.parametrize("n,s", SHAPES)
def test_lengths_have_the_symbol_size(cpu, n, s):
    """CPU: every (n, s, blob_len) the GPU tests use really has symbol size s, and the subsets
    are what their names say."""
    lens = lengths_for(cpu, n, s)
    assert set(lens) == set(LENGTH_KINDS)
    kp, ks, _ = _params(cpu, n, 1)
    for axis, k in (("primary", kp), ("secondary", ks)):
        for kind in SUBSETS:
            sel = subset(kind, n, k, seed=s)
            assert len(sel) == len(set(sel)) == k and all(0 <= i < n for i in sel)
            systematic = sum(i < k for i in sel)
            assert {"systematic": systematic == k, "no_systematic": systematic == max(0, 2 * k - n),
                    "random": 0 < systematic < k or k == 1}[kind], (n, axis, kind)


def subset(kind, n, k, seed):
    """k sliver indices of a code with k source symbols out of n."""
    if kind == "systematic":
        return list(range(k))
    if kind == "no_systematic":   # as few systematic slivers as n allows (none when n >= 2k)
        return list(range(n - k, n))
    rng = np.random.default_rng(seed * 7919 + n + k)
    while True:
        sel = [int(i) for i in rng.permutation(n)[:k]]
        if 0 < sum(i < k for i in sel) < k or k == 1:
            return sel


class Ref:
    """The C restatement's outputs for one (n, s), one encode per blob length, shared by every
    test of the shape (and dropped with it)."""

    def __init__(self, cpu, n, s):
        self.cpu, self.n, self.s = cpu, n, s
        self.kp, self.ks, _ = _params(cpu, n, 1)
        self.pl, self.sl = self.ks * s, self.kp * s
        self.lengths = lengths_for(cpu, n, s)
        self._enc, self._plan = {}, None

    def encoded(self, length):
        """(blob, primary [n][pl], secondary [n][sl], hashes [n*64], blob_id [32]) as numpy."""
        if length not in self._enc:
            n = self.n
            blob = np.random.default_rng(n * 1000 + self.s + length % 9973).integers(
                0, 256, length, dtype=np.uint8)
            prim = np.empty((n, self.pl), dtype=np.uint8)
            sec = np.empty((n, self.sl), dtype=np.uint8)
            hashes = np.empty(n * 64, dtype=np.uint8)
            bid = np.empty(32, dtype=np.uint8)
            self.cpu.rs2cpu_encode_mt(n, blob.ctypes.data, length, prim.ctypes.data,
                                      sec.ctypes.data, hashes.ctypes.data, bid.ctypes.data, 8)
            self._enc[length] = (blob, prim, sec, hashes, bid)
        return self._enc[length]

    def plan(self, gpu, length):
        """One device plan per shape, re-pointed at `length` (same symbol size)."""
        torch.cuda.synchronize()
        if self._plan is None:
            self._plan = gpu.DevicePlan(self.n, length)
        self._plan._plan.bind(length)
        return self._plan


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"n{p[0]}s{p[1]}")
def ref(request, cpu):
    r = Ref(cpu, *request.param)
    yield r
    r._enc.clear()
    r._plan = None


def _dev():
    return torch.device("cuda", 0)


def _st():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(_dev())


def _check(out, want, what, extents=None):
    out.assert_guards_intact(extents, what)                                 # A
    assert torch.equal(out.payload, want), what                             # C


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["odd_in_dword", "Lmax"])
def test_encode_guarded(gpu, ref, kind):
    """encode_async, encode_split_async and compute_metadata_async: a blob that ends inside a
    symbol at an odd byte (the zero padding is the engine's, not the caller's) and a full one."""
    n, s = ref.n, ref.s
    length = ref.lengths[kind]
    blob, prim, sec, hashes, bid = ref.encoded(length)
    plan = ref.plan(gpu, length)
    d_blob, w_prim, w_sec, w_hash, w_bid = _t(blob), _t(prim), _t(sec), _t(hashes), _t(bid)
    side = torch.cuda.Stream(_dev())
    for delta in deltas_for(n, s):
        for call in ("encode", "split", "metadata"):
            what = f"{call} n={n} s={s} blob_len={length} delta={delta}"
            outs = []
            for fill in (17, 201):
                src = Guarded(length, delta, _dev(), fill).set(d_blob)
                before = src.buf.clone()
                o_prim = Guarded(n * ref.pl, (delta + 2) % 16, _dev(), fill=90)
                o_sec = Guarded(n * ref.sl, (delta + 12) % 16, _dev(), fill=91)
                o_hash = Guarded(n * 64, 0, _dev(), fill=92)
                o_bid = Guarded(32, 0, _dev(), fill=93)
                torch.cuda.synchronize()
                if call == "encode":
                    plan.encode_async(src.ptr, o_prim.ptr, o_sec.ptr, o_hash.ptr, o_bid.ptr, _st())
                elif call == "split":
                    plan.encode_split_async(src.ptr, o_prim.ptr, o_sec.ptr, o_hash.ptr, o_bid.ptr,
                                            _st(), side.cuda_stream)
                else:
                    plan.compute_metadata_async(src.ptr, o_hash.ptr, o_bid.ptr, _st())
                torch.cuda.synchronize()
                assert torch.equal(src.buf, before), what + ": input written"
                if call == "metadata":   # the slivers stay in the plan's scratch
                    o_prim.assert_guards_intact([], what + ": d_primary")
                    o_sec.assert_guards_intact([], what + ": d_secondary")
                else:
                    _check(o_prim, w_prim, what + ": d_primary")
                    _check(o_sec, w_sec, what + ": d_secondary")
                _check(o_hash, w_hash, what + ": d_hashes")
                _check(o_bid, w_bid, what + ": d_blob_id")
                outs.append(torch.cat([o_prim.buf, o_sec.buf, o_hash.buf, o_bid.buf]))
            assert torch.equal(outs[0], outs[1]), what + ": depends on bytes outside the blob"  # B


@pytest.mark.gpu
def test_encode_batch_guarded(gpu, ref):
    """encode_batch_async: three blobs of different lengths, strided with gaps; front and back
    guards and the stride padding of the blobs' slivers, guards on d_hashes and d_blob_ids."""
    n, s = ref.n, ref.s
    lens = [ref.lengths[k] for k in ("odd_in_dword", "Lmin", "Lmax")]
    encs = [ref.encoded(length) for length in lens]
    plan = ref.plan(gpu, lens[0])
    nb = len(lens)
    bstride = ref.lengths["Lmax"] + 6
    pstride, sstride = n * ref.pl + 10, n * ref.sl + 34
    b_size = (nb - 1) * bstride + lens[-1]
    p_size, s_size = (nb - 1) * pstride + n * ref.pl, (nb - 1) * sstride + n * ref.sl
    pmask = strided_mask(p_size, nb, pstride, 1, n * ref.pl, n * ref.pl)
    smask = strided_mask(s_size, nb, sstride, 1, n * ref.sl, n * ref.sl)
    pgrid, sgrid = (torch.from_numpy(np.flatnonzero(m)).to(_dev()) for m in (pmask, smask))
    w_prim = _t(np.concatenate([e[1].reshape(-1) for e in encs]))
    w_sec = _t(np.concatenate([e[2].reshape(-1) for e in encs]))
    w_hash = _t(np.concatenate([e[3] for e in encs]))
    w_bid = _t(np.concatenate([e[4] for e in encs]))
    blobs = [_t(e[0]) for e in encs]
    for delta in deltas_for(n, s):
        what = f"batch n={n} s={s} lens={lens} delta={delta}"
        outs = []
        for fill in (17, 201):
            src = Guarded(b_size, delta, _dev(), fill)
            for b, d in enumerate(blobs):
                src.set(d, b * bstride)
            before = src.buf.clone()
            o_prim = Guarded(p_size, (delta + 2) % 16, _dev(), fill=90)
            o_sec = Guarded(s_size, (delta + 12) % 16, _dev(), fill=91)
            o_hash = Guarded(nb * n * 64, 0, _dev(), fill=92)
            o_bid = Guarded(nb * 32, 0, _dev(), fill=93)
            torch.cuda.synchronize()
            plan.encode_batch_async(nb, src.ptr, bstride, lens, o_prim.ptr, pstride, o_sec.ptr,
                                    sstride, o_hash.ptr, o_bid.ptr, _st())
            torch.cuda.synchronize()
            assert torch.equal(src.buf, before), what + ": input written"
            o_prim.assert_guards_intact(pmask, what + ": d_primary")        # A
            o_sec.assert_guards_intact(smask, what + ": d_secondary")
            assert torch.equal(o_prim.payload[pgrid], w_prim), what         # C
            assert torch.equal(o_sec.payload[sgrid], w_sec), what
            _check(o_hash, w_hash, what + ": d_hashes")
            _check(o_bid, w_bid, what + ": d_blob_ids")
            outs.append(torch.cat([o_prim.buf, o_sec.buf, o_hash.buf, o_bid.buf]))
        assert torch.equal(outs[0], outs[1]), what + ": depends on bytes outside the blobs"  # B


def _slivers(ref, length, axis):
    _, prim, sec, _, _ = ref.encoded(length)
    return (prim, ref.pl, ref.kp) if axis == "primary" else (sec, ref.sl, ref.ks)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LENGTH_KINDS)
@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_decode_guarded(gpu, ref, axis, kind):
    n, s = ref.n, ref.s
    length = ref.lengths[kind]
    blob = ref.encoded(length)[0]
    sliv, sl_len, k = _slivers(ref, length, axis)
    plan = ref.plan(gpu, length)
    d_sliv, want = _t(sliv), _t(blob)
    for sub in SUBSETS:
        sel = subset(sub, n, k, seed=s)
        offs = [i * sl_len for i in sel]
        for delta in deltas_for(n, s):
            what = f"decode {axis} n={n} s={s} blob_len={length}({kind}) from {sub} delta={delta}"
            outs = []
            for fill in (17, 201):
                src = Guarded(n * sl_len, delta, _dev(), fill).set(d_sliv)
                before = src.buf.clone()
                out = Guarded(length, (delta + 6) % 16, _dev(), fill=90)
                torch.cuda.synchronize()
                plan.decode_async(axis, sel, src.ptr, offs, out.ptr, _st())
                torch.cuda.synchronize()
                assert torch.equal(src.buf, before), what + ": input written"
                _check(out, want, what)                                     # A, C
                outs.append(out.buf)
            assert torch.equal(outs[0], outs[1]), what + ": depends on bytes outside the slivers"  # B


@pytest.mark.gpu
@pytest.mark.parametrize("check", ["default", "strict"])
def test_decode_and_verify_guarded(gpu, ref, check):
    """decode_and_verify on the device: the checks re-read the decoded blob (the default check
    rebuilds a cut last row in its own buffer; with a full last row its verifier reads the
    caller's buffer in place) and must accept it at every placement."""
    n, s = ref.n, ref.s
    for kind in ("odd_in_dword", "Lmax"):
        length = ref.lengths[kind]
        blob, _, _, hashes, bid = ref.encoded(length)
        plan = ref.plan(gpu, length)
        want = _t(blob)
        for axis, sub in (("primary", "random"), ("primary", "no_systematic"),
                          ("secondary", "random")):
            sliv, sl_len, k = _slivers(ref, length, axis)
            d_sliv = _t(sliv)
            sel = subset(sub, n, k, seed=s)
            offs = [i * sl_len for i in sel]
            for delta in deltas_for(n, s):
                what = (f"decode_and_verify {check} {axis} n={n} s={s} blob_len={length} "
                        f"from {sub} delta={delta}")
                outs = []
                for fill in (17, 201):
                    src = Guarded(n * sl_len, delta, _dev(), fill).set(d_sliv)
                    before = src.buf.clone()
                    out = Guarded(length, (delta + 6) % 16, _dev(), fill=90)
                    torch.cuda.synchronize()
                    plan.decode_and_verify(axis, sel, src.ptr, offs, hashes.tobytes(),
                                           bid.tobytes(), check, out.ptr, _st())
                    torch.cuda.synchronize()
                    assert torch.equal(src.buf, before), what + ": input written"
                    _check(out, want, what)                                 # A, C
                    outs.append(out.buf)
                assert torch.equal(outs[0], outs[1]), what                  # B


@pytest.mark.gpu
def test_plan_calls_reject_misaligned_pointers(gpu):
    """include/walrus_rs2.h: symbol-carrying buffers, offsets and strides 2-byte aligned, digest
    buffers 16-byte aligned; a violation is RS2_E_INVALID_ARGUMENT (ValueError here) on the host
    and nothing is enqueued: the buffers the calls point into stay as they were."""
    n, length = 10, 5000
    plan = gpu.DevicePlan(n, length)
    info = plan.info
    pl, sl = info.primary_sliver_len, info.secondary_sliver_len
    buf = torch.full((1 << 17,), 0x5A, dtype=torch.uint8, device=_dev())
    base = buf.data_ptr()
    assert base % 16 == 0 and n * pl <= 16384 and n * sl <= 16384
    good = dict(blob=base, prim=base + 16384, sec=base + 32768, hashes=base + 49152,
                bid=base + 53248, out=base + 57344, ids=base + 61440)
    side = torch.cuda.Stream(_dev())
    kp = info.n_primary
    sel, offs = list(range(kp)), [i * pl for i in range(kp)]
    hashes, bid = bytes(n * 64), bytes(32)

    def encode(a):
        plan.encode_async(a["blob"], a["prim"], a["sec"], a["hashes"], a["bid"], _st())

    def split(a):
        plan.encode_split_async(a["blob"], a["prim"], a["sec"], a["hashes"], a["bid"], _st(),
                                side.cuda_stream)

    def metadata(a):
        plan.compute_metadata_async(a["blob"], a["hashes"], a["bid"], _st())

    def batch(a, bs=6000, ps=None, ss=None):
        plan.encode_batch_async(2, a["blob"], bs, [length, length - 2], a["prim"],
                                ps or n * pl + 64, a["sec"], ss or n * sl + 64, a["hashes"],
                                a["ids"], _st())

    def decode(a, off=offs):
        plan.decode_async("primary", sel, a["prim"], off, a["out"], _st())

    def verify(a, off=offs):
        plan.decode_and_verify("primary", sel, a["prim"], off, hashes, bid, "skip", a["out"], _st())

    bad = []
    for call, symbol_args, digest_args in (
            (encode, ("blob", "prim", "sec"), ("hashes", "bid")),
            (split, ("blob", "prim", "sec"), ("hashes", "bid")),
            (metadata, ("blob",), ("hashes", "bid")),
            (batch, ("blob", "prim", "sec"), ("hashes", "ids")),
            (decode, ("prim", "out"), ()), (verify, ("prim", "out"), ())):
        for name in symbol_args:
            bad.append((call, dict(good, **{name: good[name] + 1}), {}))
        for name in digest_args:
            for d in (2, 4, 8):
                bad.append((call, dict(good, **{name: good[name] + d}), {}))
    bad += [(batch, good, dict(bs=6001)), (batch, good, dict(ps=n * pl + 65)),
            (batch, good, dict(ss=n * sl + 65)),
            (decode, good, dict(off=offs[:-1] + [offs[-1] + 1])),
            (verify, good, dict(off=[offs[0] + 1] + offs[1:]))]
    for call, args, kw in bad:
        with pytest.raises(ValueError, match="aligned|multiple of 2"):
            call(args, **kw)
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()), "a refused call wrote to its buffers"
