"""Helpers of the mixed sliver verification tests (tests/test_gpu_verify_mixed_*.py) -- TEST ONLY,
a plain module.  A case is a list of items (axis, symbol size, seed): sliver bytes are seeded
random (no encode is needed: the root of any K*s bytes is defined), their reference roots come
from corruption.sliver_root -- the Python oracle below n = 100, the C restatement from there on --
once per (n, size, axis, seed), shared and left unchanged.  `run` issues one
rs2_sliver_checker_verify_device_async call on torch buffers and returns what it wrote."""
import ctypes

import numpy as np
import torch

import corruption
import rs2_oracle as O
from walrus_amd import _lib

AXES = ("primary", "secondary")
SIZES = [2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258]
SIZES_1000 = [2, 20, 66, 130, 1206]
FILL = 0xEE            # outputs hold this before a call
POOL = 5               # distinct slivers per (n, size, axis): member j of a group is seed j % POOL
LAUNCHES = 6           # RS2_VERIFY_MIXED_WINDOW_LAUNCHES (include/walrus_rs2.h)
MATCH, MISMATCH, SKIPPED = _lib.RS2_SLIVER_MATCH, _lib.RS2_SLIVER_MISMATCH, _lib.RS2_SLIVER_SKIPPED


def sizes_of(n):
    return SIZES_1000 if n == 1000 else SIZES


def params(n, s):
    kp, ks = O.source_symbols_for_n_shards(n)
    return O.Rs2Params(n, kp, ks, s, kp * ks * s)


def k_of(n, axis):
    """Symbols of a sliver of `axis`: K_s for a primary sliver, K_p for a secondary one."""
    kp, ks = O.source_symbols_for_n_shards(n)
    return ks if axis == "primary" else kp


def scratch(n, s):
    """Window scratch of one sliver (include/walrus_rs2.h): n * (s + 32)."""
    return n * (s + 32)


_SLIVERS, _ROOTS = {}, {}


def sliver(n, s, axis, seed=0):
    key = (n, s, axis, seed)
    if key not in _SLIVERS:
        rng = np.random.default_rng([n, s, AXES.index(axis), seed, 1234])
        a = rng.integers(0, 256, k_of(n, axis) * s, dtype=np.uint8)
        a.setflags(write=False)
        _SLIVERS[key] = a
    return _SLIVERS[key]


def root_of(n, s, axis, data):
    """The oracle's root of arbitrary sliver bytes, cached by content."""
    raw = bytes(data)
    key = (n, s, axis, raw)
    if key not in _ROOTS:
        _ROOTS[key] = corruption.sliver_root(params(n, s), axis, raw)
    return _ROOTS[key]


def root(n, s, axis, seed=0):
    return root_of(n, s, axis, sliver(n, s, axis, seed))


def groups_case(n, sizes, per, order="interleaved", big=None):
    """Items (axis, s, seed) over sizes x both axes, `per` slivers per group (`big` = (axis, s,
    count): that group has `count` instead).  order: interleaved (A, B, A, B ...), sorted, reverse."""
    groups = [(a, s) for s in sizes for a in AXES]
    count = {g: per for g in groups}
    if big:
        count[(big[0], big[1])] = big[2]
    if order == "interleaved":
        items = [(a, s, j) for j in range(max(count.values())) for (a, s) in groups
                 if j < count[(a, s)]]
    else:
        items = [(a, s, j) for (a, s) in groups for j in range(count[(a, s)])]
        if order == "reverse":
            items.reverse()
    return [(a, s, j % POOL) for a, s, j in items]


def dev():
    return torch.device("cuda", 0)


def layout(n, items, gap=6):
    """Offsets of the items' slivers in one buffer, `gap` bytes between neighbours, and its size."""
    off, at = [], 0
    for a, s, _ in items:
        off.append(at)
        at += k_of(n, a) * s + gap
    return off, max(at - gap, 2)


def payload(n, items, off, size, data=None):
    """The buffer's bytes: every item's sliver at its offset, 0x5A between them.  data: bytes per
    item that replace the seeded ones (corrupted slivers)."""
    buf = np.full(size, 0x5A, dtype=np.uint8)
    for i, (a, s, seed) in enumerate(items):
        d = sliver(n, s, a, seed) if data is None or data[i] is None else \
            np.frombuffer(bytes(data[i]), dtype=np.uint8)
        buf[off[i]:off[i] + d.size] = d
    return buf


def expected_roots(n, items, data=None):
    return b"".join(root(n, s, a, seed) if data is None or data[i] is None
                    else root_of(n, s, a, data[i]) for i, (a, s, seed) in enumerate(items))


def stats():
    out = (ctypes.c_uint64 * 5)()
    assert _lib.lib().rs2_verify_mixed_stats(out) == 0
    return [int(x) for x in out]


def moved(before):
    return [a - b for a, b in zip(stats(), before)]


def set_budget(nbytes):
    assert _lib.lib().rs2_set_verify_mixed_budget(int(nbytes)) == 0


def call(checker, axes, sizes, base, off, expected, d_roots, d_verdict, status, stream=None):
    """The raw entry point on ctypes arrays (axes: RS2_AXIS_* values)."""
    m = len(axes)
    a_ax = (ctypes.c_uint8 * max(m, 1))(*axes)
    a_sz = (ctypes.c_uint16 * max(m, 1))(*sizes)
    a_off = (ctypes.c_uint64 * max(m, 1))(*off)
    return _lib.lib().rs2_sliver_checker_verify_device_async(
        checker.handle, m, a_ax, a_sz, base, a_off, expected, d_roots, d_verdict, status, stream)


def run(checker, n, items, expected=None, statuses=False, data=None, gap=6, stream=None):
    """One call over `items` laid out in one device buffer.  Returns (rc or statuses, roots bytes,
    verdict list or None) after a device synchronize; roots / verdicts start as FILL."""
    m = len(items)
    off, size = layout(n, items, gap)
    d_in = torch.tensor(payload(n, items, off, size, data), dtype=torch.uint8, device=dev())
    d_roots = torch.full((max(m, 1) * 32,), FILL, dtype=torch.uint8, device=dev())
    d_verdict = torch.full((max(m, 1) * 4,), FILL, dtype=torch.uint8, device=dev()) \
        if expected is not None else None
    torch.cuda.synchronize()
    out = checker.verify_async([a for a, _, _ in items], [s for _, s, _ in items], d_in.data_ptr(),
                               off, expected, d_roots.data_ptr(),
                               d_verdict.data_ptr() if d_verdict is not None else 0, stream,
                               statuses)
    torch.cuda.synchronize()
    verdict = None
    if d_verdict is not None:
        verdict = d_verdict.cpu().numpy().view(np.int32)[:m].tolist()
    return out, d_roots.cpu().numpy().tobytes()[:m * 32], verdict


def check_roots(n, items, got, data=None, what=""):
    want = expected_roots(n, items, data)
    if got == want:
        return
    bad = [i for i in range(len(items)) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    raise AssertionError(f"{what}: {len(bad)} of {len(items)} roots differ from the oracle's, the "
                         f"first at {bad[0]} {items[bad[0]]}")
