"""Containment of rs2_sliver_checker_verify_device_async (tests/guarded.py): the slivers lie in a
guarded buffer whose payload sits 0, 2, 6 and 14 bytes off the allocation's alignment, with 2-byte
gaps between them, and the last sliver ends at the payload's end; roots and verdicts go to guarded
buffers.  After the call every guard is intact, and roots and verdicts are the same under two
guard fills -- the gaps and both guards hold other bytes -- so nothing past a sliver's end feeds a
root.  Whole-call refusals enqueue nothing: sentinel-filled outputs stay untouched and the
counters do not move."""
import ctypes

import numpy as np
import pytest
import torch

import verify_mixed as M
from guarded import Guarded
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

INVALID = _lib.RS2_E_INVALID_ARGUMENT
N = 13


def _items():
    # both paths (s = 2: per-size), sizes around the chunk and Blake2b block edges, and a last
    # sliver whose final symbol ends the payload
    return M.groups_case(N, [2, 6, 62, 66, 126, 130], 2, "interleaved")


@pytest.mark.parametrize("delta", [0, 2, 6, 14])
def test_guards_and_fills(gpu, delta):
    items = _items()
    m = len(items)
    off, size = M.layout(N, items, gap=2)
    assert off[-1] + M.k_of(N, items[-1][0]) * items[-1][1] == size
    expected = M.expected_roots(N, items)
    checker = gpu.SliverChecker(N)
    results = []
    for fill in (0x11, 0xC7):
        g_in = Guarded(size, delta, M.dev(), fill)
        for i, (a, s, seed) in enumerate(items):
            g_in.set(M.sliver(N, s, a, seed).tobytes(), off[i])   # the gaps keep the pattern
        g_roots = Guarded(m * 32, 0, M.dev(), fill ^ 0x5A)
        g_verdict = Guarded(m * 4, 0, M.dev(), fill ^ 0x33)
        before_in = g_in.buf.clone()
        torch.cuda.synchronize()
        rc = checker.verify_async([a for a, _, _ in items], [s for _, s, _ in items], g_in.ptr,
                                  off, expected, g_roots.ptr, g_verdict.ptr)
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.last_error())
        g_roots.assert_guards_intact(what="d_roots")
        g_verdict.assert_guards_intact(what="d_verdict")
        assert torch.equal(g_in.buf, before_in), "the slivers' buffer was written"
        roots = g_roots.numpy().tobytes()
        M.check_roots(N, items, roots, what=f"delta {delta} fill {fill:#x}")
        verdict = g_verdict.numpy().view(np.int32).tolist()
        assert verdict == [M.MATCH] * m
        results.append((roots, verdict))
    assert results[0] == results[1]


def test_whole_call_refusals_enqueue_nothing(gpu):
    items = _items()[:6]
    m = len(items)
    off, size = M.layout(N, items, gap=2)
    expected = np.frombuffer(M.expected_roots(N, items), dtype=np.uint8)
    checker = gpu.SliverChecker(N)
    g_in = Guarded(size, 0, M.dev(), 0x21).set(M.payload(N, items, off, size))
    g_roots = Guarded(m * 32 + 16, 0, M.dev(), 0x42)
    g_verdict = Guarded(m * 4 + 16, 0, M.dev(), 0x63)
    axes = (ctypes.c_uint8 * m)(*[M.AXES.index(a) for a, _, _ in items])
    sizes = (ctypes.c_uint16 * m)(*[s for _, s, _ in items])
    offs = (ctypes.c_uint64 * m)(*off)
    exp = expected.ctypes.data
    fn = _lib.lib().rs2_sliver_checker_verify_device_async
    h = checker.handle
    torch.cuda.synchronize()
    before = M.stats()
    calls = {
        "null checker": (None, m, axes, sizes, g_in.ptr, offs, exp, g_roots.ptr, g_verdict.ptr),
        "null axis": (h, m, None, sizes, g_in.ptr, offs, exp, g_roots.ptr, g_verdict.ptr),
        "null sizes": (h, m, axes, None, g_in.ptr, offs, exp, g_roots.ptr, g_verdict.ptr),
        "null base": (h, m, axes, sizes, None, offs, exp, g_roots.ptr, g_verdict.ptr),
        "null offsets": (h, m, axes, sizes, g_in.ptr, None, exp, g_roots.ptr, g_verdict.ptr),
        "odd base": (h, m, axes, sizes, g_in.ptr + 1, offs, exp, g_roots.ptr, g_verdict.ptr),
        "roots off 16": (h, m, axes, sizes, g_in.ptr, offs, exp, g_roots.ptr + 8, g_verdict.ptr),
        "verdict off 16": (h, m, axes, sizes, g_in.ptr, offs, exp, g_roots.ptr, g_verdict.ptr + 4),
        "too many": (h, 65536, axes, sizes, g_in.ptr, offs, exp, g_roots.ptr, g_verdict.ptr),
        "expected alone": (h, m, axes, sizes, g_in.ptr, offs, exp, g_roots.ptr, None),
        "verdict alone": (h, m, axes, sizes, g_in.ptr, offs, None, g_roots.ptr, g_verdict.ptr),
    }
    for what, args in calls.items():
        assert fn(*args, None, None) == INVALID, what
    # n_slivers 0 is RS2_OK and enqueues nothing either
    assert fn(h, 0, None, None, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert M.moved(before) == [0] * 5
    g_roots.assert_guards_intact(extents=[], what="d_roots")
    g_verdict.assert_guards_intact(extents=[], what="d_verdict")
    # and the checker still works
    rc, roots, _ = M.run(checker, N, items)
    assert rc == 0
    M.check_roots(N, items, roots, what="after the refusals")
