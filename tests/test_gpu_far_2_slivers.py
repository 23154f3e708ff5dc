"""The per-sliver calls of a storage node at large symbols, n = 1000: symbol sizes one step either
side of the planner's span switch and the largest one.

A sliver's codec job has the line stride max(K, n - K) * s.  plan_sliver_groups / finish_plan
(rs2_planner.cpp) give it an even pairs_span while that is below T = (2^31 - 65536) / 64 =
33,553,408 bytes and a multiple of 64 from T on (test_gpu_far_1_codec1d.py).  At n = 1000 a primary
sliver (K = 667) crosses T between s = 50,304 and 50,306, a secondary one (K = 334, n - K = 666)
between 50,380 and 50,382: blobs of about 11.2 GB and more, up to the largest symbol 65,534.  The
other sliver-level tests stop at s = 1,206.  Here the sizes LARGE run through

  rs2_verifier_roots_device_async, rs2_verifier_recovery_symbols_multi_device_async and
  rs2_verifier_recover_slivers_device_async, one (axis, size) per test, and
  rs2_sliver_checker_verify_device_async, ..._recovery_symbols_device_async and
  ..._recover_device_async with the large groups (two slivers each) interleaved with groups of
  s = 66 and 1,206 (three slivers each) on both axes, so one launch holds groups of both span
  kinds and tiny groups beside 40 MB ones.

Slivers are verify_mixed.sliver's seeded random K * s bytes.  Every expected byte comes from the C
restatement (oracle/rs2_cpu.c) through tests/corruption.py: sliver_root, recovery_symbol (targets
0, K - 1, K, K + 1, n - 1: symbol and proof), expand_sliver + recover_sliver (from the last K of
the n expanded symbols -- no systematic symbol on the secondary axis; on the primary one, whose
code has 333 repairs for K = 667, all of those and the fewest systematic ones, 334 -- and from a seeded
random K-subset; the recovered bytes are also the original sliver's).  Each reference is computed once, on a small
thread pool, and shared through the module's caches.  Outputs start as FILL and the 64 bytes past
each documented extent must keep it.  tests/test_planner_span.py asserts on the CPU which span
each (axis, size) of this file gets.  No test holds 2 GiB of device memory."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import corruption
import verify_mixed as M

N = 1000
AXES = M.AXES
LARGE = {"primary": (50304, 50306, 65534), "secondary": (50380, 50382, 65534)}
SMALL = (66, 1206)
PER_LARGE, PER_SMALL = 2, 3
# the mixed calls' groups in order of first appearance: both span kinds and both small sizes on
# both axes
GROUPS = [("primary", 50304), ("primary", 66), ("secondary", 50380), ("secondary", 1206),
          ("primary", 50306), ("secondary", 66), ("secondary", 50382), ("primary", 1206),
          ("primary", 65534), ("secondary", 65534)]
FILL, PAST = 0xEE, 64
PATH = 10                       # Merkle path of 1000 leaves
BUDGET = 1 << 30                # one verify window takes all 24 slivers (0.7 GB of scratch)
MATCH, MISMATCH = M.MATCH, M.MISMATCH
PER_SIZE = [pytest.param(a, s, id=f"{a}-s{s}") for a in AXES for s in LARGE[a]]


def k_of(axis):
    return M.k_of(N, axis)


def targets(axis):
    k = k_of(axis)
    return [0, k - 1, k, k + 1, N - 1]


def mixed_items():
    """(axis, s, seed), the groups' members dealt round-robin (A0, B0, ..., A1, B1, ...)."""
    count = {g: PER_SMALL if g[1] in SMALL else PER_LARGE for g in GROUPS}
    return [(a, s, j) for j in range(PER_SMALL) for (a, s) in GROUPS if j < count[(a, s)]]


def subset(axis, s, seed, kind):
    """Indices of the K received symbols: the last K of n, or a seeded random K-subset in the
    order it is handed over."""
    k = k_of(axis)
    if kind == "last":
        return list(range(N - k, N))
    rng = np.random.default_rng([s, AXES.index(axis), seed, 4242])
    return [int(q) for q in rng.permutation(N)[:k]]


# ---- references: the C restatement, once per key -------------------------------------------------
_ROOTS, _SYMBOLS, _EXPANDED, _RECOVERED = {}, {}, {}, {}


def _data(axis, s, seed):
    return M.sliver(N, s, axis, seed)


def _root(key):
    axis, s, seed = key
    return corruption.sliver_root(M.params(N, s), axis, _data(*key))


def _symbol(key):
    axis, s, seed, t = key
    return corruption.recovery_symbol(M.params(N, s), axis, _data(axis, s, seed), t)


def _expanded(key):
    axis, s, seed = key
    ex = corruption.expand_sliver(M.params(N, s), axis, _data(*key))
    assert ex[:k_of(axis)].tobytes() == _data(*key).tobytes()   # systematic
    ex.setflags(write=False)
    return ex


def _recovered(key):
    axis, s, seed, kind = key
    idx = subset(axis, s, seed, kind)
    got, root = corruption.recover_sliver(M.params(N, s), axis, idx, _EXPANDED[(axis, s, seed)][idx])
    assert got == _data(axis, s, seed).tobytes(), key       # the reference's own round trip
    return root


def _warm(cache, fn, keys):
    """cache[key] = fn(key) for the missing keys, eight at a time (the C restatement keeps its
    state per thread and ctypes releases the interpreter lock)."""
    todo = [k for k in dict.fromkeys(keys) if k not in cache]
    if todo:
        # the restatement's tables are built in place on first use, which two threads must not
        # do at once: build them here, before the pool starts
        corruption._cpu_lib().rs2cpu_init()
        with ThreadPoolExecutor(max_workers=8) as pool:
            for k, v in zip(todo, pool.map(fn, todo)):
                cache[k] = v
    return [cache[k] for k in keys]


def roots_of(items):
    return b"".join(_warm(_ROOTS, _root, [tuple(it[:3]) for it in items]))


def recovered_roots(items, kinds):
    _warm(_EXPANDED, _expanded, [tuple(it[:3]) for it in items])
    return b"".join(_warm(_RECOVERED, _recovered, [tuple(it[:3]) + (kd,)
                                                   for it, kd in zip(items, kinds)]))


# ---- device buffers -------------------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


def filled(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev())


def packed(chunks, gap):
    """The chunks (numpy byte arrays) in one device buffer, `gap` bytes of 0x5A between and after
    them: (tensor, offsets)."""
    off, at = [], 0
    for c in chunks:
        off.append(at)
        at += c.size + gap
    host = np.full(max(at, 2), 0x5A, dtype=np.uint8)
    for o, c in zip(off, chunks):
        host[o:o + c.size] = c.reshape(-1)
    return torch.from_numpy(host).to(dev()), off


def out_layout(lengths):
    """Output extents PAST bytes apart: (offsets, total bytes)."""
    off, at = [], 0
    for ln in lengths:
        off.append(at)
        at += ln + PAST
    return off, max(at, 2)


def check_extents(buf, off, want, what, s=None):
    """Each extent equals want[i]; every other byte -- PAST of them after each -- is still FILL.
    s: the extents hold symbols of s bytes (a failure names the wrong symbols and their bytes)."""
    host = buf.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for i, (o, w) in enumerate(zip(off, want)):
        keep[o:o + len(w)] = False
        got = host[o:o + len(w)]
        if got.tobytes() != bytes(w):
            bad = np.flatnonzero(got != np.frombuffer(bytes(w), dtype=np.uint8))
            detail = ""
            if s:
                sym = bad // s
                which = np.unique(sym)
                spans = [(int(q), int(bad[sym == q].min() % s), int(bad[sym == q].max() % s),
                          int((sym == q).sum())) for q in which[:12]]
                detail = (f"; {which.size} symbols of {s} bytes are wrong, (symbol, first byte, "
                          f"last byte, bytes) of the first: {spans}, the last symbol {int(which[-1])}")
            raise AssertionError(f"{what}: extent {i}: {bad.size} of {len(w)} bytes differ from the "
                                 f"reference's, the first at {int(bad[0])}{detail}")
    assert (host[keep] == FILL).all(), f"{what}: bytes outside the documented extents were written"


def verdicts(buf, m):
    return buf.cpu().numpy()[:4 * m].view(np.int32).tolist()


def flipped(roots, i):
    b = bytearray(roots)
    b[32 * i + 5] ^= 0x40
    return bytes(b)


# ---- verification ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("axis,s", PER_SIZE)
def test_roots_per_size(gpu, axis, s):
    items = [(axis, s, j) for j in range(PER_LARGE)]
    want = roots_of(items)
    d_sl, _ = packed([_data(*it) for it in items], 0)
    d_roots = filled(32 * len(items) + PAST)
    v = gpu.SliverVerifier(N, s, axis)
    torch.cuda.synchronize()     # the call runs on the verifier's stream, not on torch's
    v.roots_async(len(items), d_sl.data_ptr(), d_roots.data_ptr())
    torch.cuda.synchronize()
    check_extents(d_roots, [0], [want], f"roots {axis} s={s}")


@pytest.mark.gpu
def test_verify_mixed(gpu):
    items = mixed_items()
    m = len(items)
    want = roots_of(items)
    wrong = next(i for i, it in enumerate(items) if it[:2] == ("primary", 50306))
    d_sl, off = packed([_data(*it) for it in items], 6)
    d_roots, d_verdict = filled(32 * m + PAST), filled(4 * m + PAST)
    checker = gpu.SliverChecker(N)
    torch.cuda.synchronize()     # the call runs on the checker's stream, not on torch's
    M.set_budget(BUDGET)
    try:
        before = M.stats()
        rc = checker.verify_async([a for a, _, _ in items], [s for _, s, _ in items],
                                  d_sl.data_ptr(), off, flipped(want, wrong), d_roots.data_ptr(),
                                  d_verdict.data_ptr())
        torch.cuda.synchronize()
        moved = M.moved(before)
    finally:
        M.set_budget(0)
    assert rc == 0
    check_extents(d_roots, [0], [want], "mixed verify roots")
    assert verdicts(d_verdict, m) == [MISMATCH if i == wrong else MATCH for i in range(m)]
    assert (d_verdict[4 * m:] == FILL).all()
    # one window; every sliver, the large groups included, inside the group launches and none on
    # the per-size path; a group per (axis, size)
    assert moved[:4] == [1, m, 0, len(GROUPS)], moved


# ---- recovery symbols (BUILD) ---------------------------------------------------------------------
def _want_symbols(items):
    keys = [tuple(it) + (t,) for it in items for t in targets(it[0])]
    got = _warm(_SYMBOLS, _symbol, keys)
    per = len(targets("primary"))
    sym = [b"".join(x[0] for x in got[i * per:(i + 1) * per]) for i in range(len(items))]
    assert all(len(x[1]) == 32 * PATH for x in got)
    return sym, b"".join(x[1] for x in got)


@pytest.mark.gpu
@pytest.mark.parametrize("axis,s", PER_SIZE)
def test_recovery_symbols_per_size(gpu, axis, s):
    items = [(axis, s, j) for j in range(PER_LARGE)]
    sym, prf = _want_symbols(items)
    d_sl, _ = packed([_data(*it) for it in items], 0)
    d_sym, d_prf = filled(len(b"".join(sym)) + PAST), filled(len(prf) + PAST)
    v = gpu.SliverVerifier(N, s, axis)
    torch.cuda.synchronize()     # the call runs on the verifier's stream, not on torch's
    rc = v.recovery_symbols_multi_async(
        d_sl.data_ptr(), [targets(axis)] * len(items), d_sym.data_ptr(), d_prf.data_ptr(), 0, "build")
    torch.cuda.synchronize()
    assert rc == 0
    check_extents(d_sym, [0], [b"".join(sym)], f"symbols {axis} s={s}")
    check_extents(d_prf, [0], [prf], f"proofs {axis} s={s}")


@pytest.mark.gpu
def test_recovery_symbols_mixed(gpu):
    items = mixed_items()
    sym, prf = _want_symbols(items)
    d_sl, i_off = packed([_data(*it) for it in items], 2)
    before = d_sl.clone()
    o_off, o_size = out_layout([len(x) for x in sym])
    d_sym, d_prf = filled(o_size), filled(len(prf) + PAST)
    checker = gpu.SliverChecker(N)
    torch.cuda.synchronize()     # the call runs on the checker's stream, not on torch's
    rc = checker.recovery_symbols_async(
        [a for a, _, _ in items], [s for _, s, _ in items], d_sl.data_ptr(), i_off,
        [targets(a) for a, _, _ in items], d_sym.data_ptr(), o_off, d_prf.data_ptr(), 0, "build")
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(d_sl, before), "the sliver buffer was written"
    check_extents(d_sym, o_off, sym, "mixed symbols")
    check_extents(d_prf, [0], [prf], "mixed proofs")


# ---- recovery -------------------------------------------------------------------------------------
def _received(items, kinds):
    return [_EXPANDED[tuple(it[:3])][subset(*it[:3], kd)] for it, kd in zip(items, kinds)]


@pytest.mark.gpu
@pytest.mark.parametrize("axis,s", PER_SIZE)
def test_recover_per_size(gpu, axis, s):
    """Both slivers from their last K symbols and from a random K-subset: four recoveries."""
    items = [(axis, s, j) for j in range(PER_LARGE)] * 2
    kinds = ["last"] * PER_LARGE + ["random"] * PER_LARGE
    m = len(items)
    want = recovered_roots(items, kinds)
    assert want == roots_of(items)
    d_sym, _ = packed(_received(items, kinds), 0)
    before = d_sym.clone()
    ln = k_of(axis) * s
    d_out, d_roots, d_verdict = filled(m * ln + PAST), filled(32 * m + PAST), filled(4 * m + PAST)
    v = gpu.SliverVerifier(N, s, axis)
    torch.cuda.synchronize()     # the call runs on the verifier's stream, not on torch's
    rc = v.recover_slivers_async(
        [subset(*it, kd) for it, kd in zip(items, kinds)], d_sym.data_ptr(), d_out.data_ptr(),
        flipped(want, 2), d_roots.data_ptr(), d_verdict.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(d_sym, before), "the symbol buffer was written"
    check_extents(d_out, [0], [b"".join(_data(*it).tobytes() for it in items)],
                  f"recovered {axis} s={s}", s)
    check_extents(d_roots, [0], [want], f"recovered roots {axis} s={s}")
    assert verdicts(d_verdict, m) == [MATCH, MATCH, MISMATCH, MATCH]
    assert (d_verdict[4 * m:] == FILL).all()


@pytest.mark.gpu
def test_recover_mixed(gpu):
    """Every sliver of the mixed list once, the two subset kinds alternating inside each group."""
    items = mixed_items()
    kinds = ["last" if (seed + GROUPS.index((a, s))) % 2 == 0 else "random" for a, s, seed in items]
    m = len(items)
    want = recovered_roots(items, kinds)
    assert want == roots_of(items)
    wrong = next(i for i, it in enumerate(items) if it[:2] == ("secondary", 50382))
    d_sym, s_off = packed(_received(items, kinds), 2)
    before = d_sym.clone()
    o_off, o_size = out_layout([k_of(a) * s for a, s, _ in items])
    d_out, d_roots, d_verdict = filled(o_size), filled(32 * m + PAST), filled(4 * m + PAST)
    checker = gpu.SliverChecker(N)
    torch.cuda.synchronize()     # the call runs on the checker's stream, not on torch's
    rc = checker.recover_async(
        [a for a, _, _ in items], [s for _, s, _ in items],
        [subset(*it, kd) for it, kd in zip(items, kinds)], d_sym.data_ptr(), s_off,
        d_out.data_ptr(), o_off, flipped(want, wrong), d_roots.data_ptr(), d_verdict.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(d_sym, before), "the symbol buffer was written"
    check_extents(d_out, o_off, [_data(*it).tobytes() for it in items], "mixed recovered")
    check_extents(d_roots, [0], [want], "mixed recovered roots")
    assert verdicts(d_verdict, m) == [MISMATCH if i == wrong else MATCH for i in range(m)]
    assert (d_verdict[4 * m:] == FILL).all()


# ---- the case lists themselves (CPU) --------------------------------------------------------------
def test_sizes_and_groups_are_what_they_claim():
    T = (2 ** 31 - 65536) // 64
    for axis in AXES:
        k = k_of(axis)
        far = max(k, N - k)
        below, above, top = LARGE[axis]
        assert above == below + 2 and far * below < T <= far * above and top == 65534
        assert targets(axis) == sorted(set(targets(axis))) and targets(axis)[-1] == N - 1
        for s in LARGE[axis]:
            for seed in range(PER_LARGE):
                idx = subset(axis, s, seed, "random")
                assert len(set(idx)) == k and idx != sorted(idx) and any(q < k for q in idx)
            # no systematic symbol where the code has K repairs (secondary); else every repair
            last = subset(axis, s, 0, "last")
            assert last == list(range(N - k, N))
            assert (min(last) >= k) == (axis == "secondary") == (N - k >= k)
            assert sum(q >= k for q in last) == min(k, N - k)
    assert (k_of("primary"), k_of("secondary")) == (667, 334)
    items = mixed_items()
    assert len(items) == 6 * PER_LARGE + 4 * PER_SMALL == 24
    assert {it[:2] for it in items} == set(GROUPS) == \
        {(a, s) for a in AXES for s in LARGE[a] + SMALL}
    assert [it[:2] for it in items[:len(GROUPS)]] == GROUPS            # dealt round-robin
    # device memory: slivers + window scratch of the one-window verify, inputs + outputs +
    # default-budget scratch of the mixed recovery, four in and four out of the per-size one
    slivers = sum(k_of(a) * s for a, s, _ in items)
    scratch = sum(M.scratch(N, s) for _, s, _ in items)
    assert scratch <= BUDGET and slivers + scratch < 3 << 29
    assert 2 * slivers + (256 << 20) + M.scratch(N, 65534) < 3 << 29
    assert 8 * 667 * 65534 + (256 << 20) + M.scratch(N, 65534) < 3 << 29
