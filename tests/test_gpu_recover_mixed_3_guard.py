"""Containment of the mixed recovery calls (tests/guarded.py): the received symbols and the output
slivers lie in guarded buffers whose payloads sit 0, 2, 6 and 14 bytes off the allocation's
alignment; neighbouring output slivers are 2 or 6 bytes apart (odd multiples of 2), the last one
ends at the payload's end; roots, verdicts and the proof check's flags go to guarded buffers.
After the call every guard and every gap is intact, the symbol buffer is unchanged, and the
results are the same under two guard fills, so nothing outside a sliver's symbols feeds its
output.  Whole-call refusals enqueue nothing: sentinel-filled outputs stay untouched and the
counters do not move."""
import ctypes

import numpy as np
import pytest
import torch

import recover_mixed as R
import rs2_oracle as O
import verify_mixed as M
from guarded import Guarded
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

INVALID = _lib.RS2_E_INVALID_ARGUMENT
N = 13


def _items():
    # batched and per-sliver decodes (s = 2; every original received), sizes round the tile and
    # Blake2b block edges
    items = R.family_case(N, [2, 6, 62, 64, 66, 126, 128, 130, 254, 258], only_batched=False)[:32]
    items.insert(5, ("primary", 66, list(range(R.k_of(N, "primary"))), 1))
    return items


@pytest.mark.parametrize("delta,gap", [(0, 2), (2, 6), (6, 2), (14, 6)])
def test_guards_gaps_and_fills(gpu, delta, gap):
    items = _items()
    m = len(items)
    s_off, s_size, o_off, o_size = R.layout(N, items, gap)
    assert o_off[-1] + R.k_of(N, items[-1][0]) * items[-1][1] == o_size
    assert all(o % 2 == 0 for o in o_off) and any(o % 4 == 2 for o in o_off)
    extents = [(o_off[i], R.k_of(N, it[0]) * it[1]) for i, it in enumerate(items)]
    expected = R.expected_roots(N, items)
    checker = gpu.SliverChecker(N)
    results = []
    for fill in (0x11, 0xC7):
        g_sym = Guarded(s_size, delta, R.dev(), fill)
        for i, it in enumerate(items):
            g_sym.set(R.received(N, it), s_off[i])           # the gaps keep the pattern
        g_out = Guarded(o_size, (delta + 4) % 16, R.dev(), fill ^ 0x77)
        g_roots = Guarded(m * 32, 0, R.dev(), fill ^ 0x5A)
        g_verdict = Guarded(m * 4, 0, R.dev(), fill ^ 0x33)
        before = g_sym.buf.clone()
        torch.cuda.synchronize()
        rc = checker.recover_async([a for a, _, _, _ in items], [s for _, s, _, _ in items],
                                   [p for _, _, p, _ in items], g_sym.ptr, s_off, g_out.ptr, o_off,
                                   expected, g_roots.ptr, g_verdict.ptr)
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.last_error())
        g_out.assert_guards_intact(extents=extents, what="d_slivers")
        g_roots.assert_guards_intact(what="d_roots")
        g_verdict.assert_guards_intact(what="d_verdict")
        assert torch.equal(g_sym.buf, before), "the symbol buffer was written"
        out = g_out.numpy()
        for i, it in enumerate(items):
            o, ln = extents[i]
            assert out[o:o + ln].tobytes() == R.want_sliver(N, it), (i, it[:2])
        roots = g_roots.numpy().tobytes()
        assert roots == expected
        verdict = g_verdict.numpy().view(np.int32).tolist()
        assert verdict == [R.MATCH] * m
        results.append((out[[b for o, ln in extents for b in range(o, o + ln)]].tobytes(), roots,
                        verdict))
    assert results[0] == results[1]


@pytest.mark.parametrize("delta", [0, 6])
def test_proof_check_guards(gpu, delta):
    sizes, counts, targets = [4, 62, 130, 258], [3, 1, 4, 2], [0, 5, 12, 7]
    L = len(O.merkle_proof([b"\0\0"] * N, 0))
    runs, proofs, roots = [], [], []
    for g, (s, c, t) in enumerate(zip(sizes, counts, targets)):
        run = b""
        for j in range(c):
            leaves = [bytes(x) for x in R.codeword(N, s, R.AXES[g % 2], j)]
            run += leaves[t]
            proofs.append(b"".join(O.merkle_proof(leaves, t)))
            roots.append(O.merkle_root(leaves))
        runs.append(run)
    off, at = [], 0
    for r in runs:
        off.append(at)
        at += len(r) + 2
    total = sum(counts)
    results = []
    for fill in (0x11, 0xC7):
        g_sym = Guarded(at - 2, delta, R.dev(), fill)
        for o, r in zip(off, runs):
            g_sym.set(r, o)
        g_proofs = Guarded(total * L * 32, 0, R.dev(), fill ^ 1).set(b"".join(proofs))
        g_roots = Guarded(total * 32, 0, R.dev(), fill ^ 2).set(b"".join(roots))
        g_ok = Guarded(total, 0, R.dev(), fill ^ 0x44)
        before = [g.buf.clone() for g in (g_sym, g_proofs, g_roots)]
        torch.cuda.synchronize()
        rc = gpu.SliverChecker(N).check_recovery_symbols_async(
            sizes, counts, targets, g_sym.ptr, off, g_proofs.ptr, g_roots.ptr, g_ok.ptr)
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.last_error())
        g_ok.assert_guards_intact(what="d_ok")
        for g, b in zip((g_sym, g_proofs, g_roots), before):
            assert torch.equal(g.buf, b), "an input of the proof check was written"
        results.append(g_ok.numpy().tolist())
    assert results[0] == results[1] == [1] * total


def test_whole_call_refusals_enqueue_nothing(gpu):
    items = _items()[:6]
    m = len(items)
    s_off, s_size, o_off, o_size = R.layout(N, items, 2)
    expected = np.frombuffer(R.expected_roots(N, items), dtype=np.uint8)
    checker = gpu.SliverChecker(N)
    g_sym = Guarded(s_size, 0, R.dev(), 0x21).set(R.payload(N, items, s_off, s_size))
    g_out = Guarded(o_size, 0, R.dev(), 0x35)
    g_roots = Guarded(m * 32 + 16, 0, R.dev(), 0x42)
    g_verdict = Guarded(m * 4 + 16, 0, R.dev(), 0x63)
    axes = (ctypes.c_uint8 * m)(*[R.AXES.index(a) for a, _, _, _ in items])
    sizes = (ctypes.c_uint16 * m)(*[s for _, s, _, _ in items])
    counts = (ctypes.c_uint32 * m)(*[len(p) for _, _, p, _ in items])
    flat = [q for _, _, p, _ in items for q in p]
    idx = (ctypes.c_uint16 * len(flat))(*flat)
    so, oo = (ctypes.c_uint64 * m)(*s_off), (ctypes.c_uint64 * m)(*o_off)
    exp = expected.ctypes.data
    fn = _lib.lib().rs2_sliver_checker_recover_device_async
    h = checker.handle
    good = [h, m, axes, sizes, counts, idx, g_sym.ptr, so, exp, g_out.ptr, oo, g_roots.ptr,
            g_verdict.ptr]

    def but(**kw):
        names = ["c", "m", "axes", "sizes", "counts", "idx", "sym", "so", "exp", "out", "oo", "roots",
                 "verdict"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args

    torch.cuda.synchronize()
    before, before_vm = R.stats(), M.stats()
    calls = {
        "null checker": but(c=None), "null axis": but(axes=None), "null sizes": but(sizes=None),
        "null counts": but(counts=None), "null indices": but(idx=None),
        "null symbols": but(sym=None), "null symbol offsets": but(so=None),
        "null output": but(out=None), "null output offsets": but(oo=None),
        "odd symbol base": but(sym=g_sym.ptr + 1), "odd output base": but(out=g_out.ptr + 1),
        "roots off 16": but(roots=g_roots.ptr + 8), "verdict off 16": but(verdict=g_verdict.ptr + 4),
        "too many": but(m=65536), "expected alone": but(verdict=None),
        "verdict alone": but(exp=None),
    }
    for what, args in calls.items():
        assert fn(*args, None, None) == INVALID, what
    assert fn(h, 0, *([None] * 13)) == 0               # n_slivers 0: RS2_OK, nothing enqueued
    torch.cuda.synchronize()
    assert R.moved(before) == [0] * 5 and M.moved(before_vm) == [0] * 5
    g_out.assert_guards_intact(extents=[], what="d_slivers")
    g_roots.assert_guards_intact(extents=[], what="d_roots")
    g_verdict.assert_guards_intact(extents=[], what="d_verdict")
    # and the checker still works
    rc, out, off, roots, _ = R.run(checker, N, items)
    assert rc == 0
    R.check_slivers(N, items, out, off, what="after the refusals")
    R.check_roots(N, items, roots, what="after the refusals")
