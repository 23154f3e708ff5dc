"""Helpers of the mixed recovery-symbol tests (tests/test_gpu_symbols_mixed_*.py) -- TEST ONLY, a
plain module built on symbols_multi.py.  A case is a list of items (axis, symbol size, pool index,
targets): the source sliver is number `pool index` of symbols_multi.reference(n, size, axis, POOL)
-- seeded random bytes expanded and hashed by the oracle once per (n, size, axis), shared and left
unchanged -- and what the call must write for it is symbols_multi.expected, never the call under
test.  `run` issues one rs2_sliver_checker_recovery_symbols_device_async call on torch buffers and
returns what it wrote; `run_per_size` the same requests through one
rs2_verifier_recovery_symbols_multi_device_async call per (axis, size); `predicted` restates the
plan's counters in Python."""
import ctypes

import numpy as np
import torch

import symbols_multi as SM
from walrus_amd import _lib

AXES = SM.AXES
POOL = 3
FILL = 0xEE
INVALID = _lib.RS2_E_INVALID_ARGUMENT
WINDOW_GROUPS = 256          # RS2_VERIFY_MIXED_WINDOW_GROUPS
WINDOW_LAUNCHES = 7          # RS2_SYMBOLS_MIXED_WINDOW_LAUNCHES
GROUP_MAX_LEAVES = 4096
REQUEST_CHUNK = 1 << 20     # requests of one gather launch
k_of, shape, dev, to_dev = SM.k_of, SM.shape, SM.dev, SM.to_dev


def ref_of(n, item, cpu=None, pool=POOL):
    return SM.reference(n, item[1], item[0], pool, cpu=cpu)


def stats():
    out = (ctypes.c_uint64 * 6)()
    assert _lib.lib().rs2_symbols_mixed_stats(out) == 0
    return [int(x) for x in out]


def moved(before):
    return [a - b for a, b in zip(stats(), before)]


def want(n, items, cpu=None, pool=POOL):
    """Per item (symbols, proofs, nodes) from the oracle, as bytes."""
    out = []
    for it in items:
        ref = ref_of(n, it, cpu, pool)
        per = [[] for _ in range(pool)]
        per[it[2]] = list(it[3])
        sym, prf = SM.expected(ref, per)
        out.append((sym.tobytes(), prf.tobytes(), ref["nodes"][it[2]].tobytes()))
    return out


def layout(n, items, in_gap=2, out_gap=6):
    """(sliver offsets, sliver bytes, symbol offsets, symbol bytes): slivers `in_gap` bytes apart,
    the slivers' symbol extents `out_gap` bytes apart."""
    i_off, o_off, ia, oa = [], [], 0, 0
    for a, s, _, ts in items:
        i_off.append(ia)
        o_off.append(oa)
        ia += k_of(n, a) * s + in_gap
        oa += len(ts) * s + out_gap
    return i_off, max(ia, 2), o_off, max(oa, 2)


def payload(n, items, i_off, size, cpu=None, pool=POOL, fill=0x5A):
    buf = np.full(size, fill, dtype=np.uint8)
    for it, o in zip(items, i_off):
        d = ref_of(n, it, cpu, pool)["data"][it[2]]
        buf[o:o + d.size] = d
    return buf


def eligible(n, s):
    """Whether a group of symbol size s runs inside the group launches (the default block limit:
    every code of n <= 4096 has at most 8 transform blocks)."""
    return s >= 4 and n <= GROUP_MAX_LEAVES


def windows(n, items, budget, build, accepted=None):
    """The window rule restated: lists of item indices (accepted ones)."""
    _, nn = shape(n)
    out, cur, used, groups = [], [], 0, set()
    for i, (a, s, _, _) in enumerate(items):
        if accepted is not None and not accepted[i]:
            continue
        need = n * (s + 32) + (nn * 32 if build else 0)
        if cur and (used + need > budget or ((a, s) not in groups and len(groups) == WINDOW_GROUPS)):
            out.append(cur)
            cur, used, groups = [], 0, set()
        cur.append(i)
        used += need
        groups.add((a, s))
    out.append(cur)
    return out


def predicted(n, items, trees="build", have_nodes=False, budget=256 << 20, accepted=None):
    """[windows, expanded, built, cached, requests, launches] a call adds."""
    build = trees == "build"
    wins = [w for w in windows(n, items, budget, build, accepted) if w]  # none: all refused
    expanded = built = cached = requests = launches = 0
    for win in wins:
        ex = []
        for i in win:
            a, s, _, ts = items[i]
            if (build and (have_nodes or ts)) or (not build and any(t >= k_of(n, a) for t in ts)):
                ex.append(i)
            requests += len(ts)
            cached += (not build) and len(ts) > 0
        expanded += len(ex)
        built += len(ex) if build else 0
        el = [i for i in ex if eligible(n, items[i][1])]
        launches += 1 if ex else 0                                  # gather
        launches += len({items[i][0] for i in el})                  # encode groups, one per axis
        if build and ex:
            launches += (1 if el else 0) + (1 if n <= GROUP_MAX_LEAVES else 0)   # leaves, trees
            launches += 1 if have_nodes else 0                      # scatter
        served = sum(len(items[i][3]) for i in win)
        # the window's requests in chunks, refused slivers' entries between accepted ones included
        span = sum(len(items[i][3]) for i in range(min(win), max(win) + 1))
        launches += -(-span // REQUEST_CHUNK) if served else 0
    return [len(wins), expanded, built, cached, requests, launches]


def call_raw(checker, items, d_slivers, i_off, d_sym, o_off, d_prf, d_nodes, trees, stream=None,
             statuses=False, rewrite=True):
    """The C call on arrays of this function's own, overwritten with other values as soon as it
    returns (the host arrays are free then).  Returns rc, or the status list."""
    m = len(items)
    ax = np.array([AXES.index(a) if a in AXES else a for a, _, _, _ in items] + [0], dtype=np.uint8)
    sz = np.array([s for _, s, _, _ in items] + [0], dtype=np.uint16)
    counts = np.array([len(t) for _, _, _, t in items] + [0], dtype=np.uint32)
    tg = np.array([t for _, _, _, ts in items for t in ts] + [0], dtype=np.uint16)
    io = np.array(list(i_off) + [0], dtype=np.uint64)
    oo = np.array(list(o_off) + [0], dtype=np.uint64)
    st = (ctypes.c_int * max(m, 1))() if statuses else None
    u16, u32, u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64))
    mode = {"build": _lib.RS2_TREES_BUILD, "cached": _lib.RS2_TREES_CACHED}.get(trees, trees)
    rc = _lib.lib().rs2_sliver_checker_recovery_symbols_device_async(
        checker.handle, m, ax.ctypes.data, sz.ctypes.data_as(u16), d_slivers or None,
        io.ctypes.data_as(u64), counts.ctypes.data_as(u32), tg.ctypes.data_as(u16), mode,
        d_nodes or None, d_sym or None, oo.ctypes.data_as(u64), d_prf or None, st,
        ctypes.c_void_p(stream) if stream else None)
    if rewrite:
        ax[:], sz[:], counts[:], tg[:], io[:], oo[:] = 1, 2, 1, 0, 0, 0
    if statuses:
        assert rc == 0, _lib.last_error()
        return list(st)[:m]
    return rc


def run(checker, n, items, trees="build", nodes=None, want_nodes=False, stream=None,
        statuses=False, cpu=None, pool=POOL):
    """One call over `items`.  nodes: a device tensor holding the trees in the caller's order
    (CACHED, or BUILD into it); want_nodes: BUILD into a fresh filled buffer.  Returns (rc or
    statuses, symbol buffer, symbol offsets, proofs, nodes) as numpy after a synchronize; outputs
    start as FILL; the sliver buffer must come back unchanged."""
    L, nn = shape(n)
    m = len(items)
    total = sum(len(t) for _, _, _, t in items)
    i_off, i_size, o_off, o_size = layout(n, items)
    d_sl = torch.tensor(payload(n, items, i_off, i_size, cpu, pool), dtype=torch.uint8, device=dev())
    before = d_sl.clone()
    d_sym = torch.full((o_size,), FILL, dtype=torch.uint8, device=dev())
    d_prf = torch.full((max(total * L * 32, 32),), FILL, dtype=torch.uint8, device=dev())
    if nodes is None and want_nodes:
        nodes = torch.full((m * nn * 32,), FILL, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    res = call_raw(checker, items, d_sl.data_ptr(), i_off, d_sym.data_ptr(), o_off, d_prf.data_ptr(),
                   nodes.data_ptr() if nodes is not None else 0, trees, stream, statuses)
    torch.cuda.synchronize()
    assert torch.equal(d_sl, before), "the sliver buffer was written"
    return (res, d_sym.cpu().numpy(), o_off, d_prf.cpu().numpy()[:total * L * 32],
            None if nodes is None else nodes.cpu().numpy())


def check_outputs(n, items, sym, o_off, prf, nodes=None, skipped=(), cpu=None, pool=POOL, what="",
                  nodes_written=True):
    """Every accepted item's symbols, proofs (and trees) equal the oracle's; a skipped item's
    symbol extent, proof slots and node slot, and every gap, still hold FILL."""
    L, nn = shape(n)
    keep = np.ones(sym.size, dtype=bool)
    j = 0
    for i, it in enumerate(items):
        cnt, s = len(it[3]), it[1]
        if i not in skipped:
            w_sym, w_prf, w_nodes = want(n, [it], cpu, pool)[0]
        got_prf = prf[j * L * 32:(j + cnt) * L * 32].tobytes()
        if i in skipped:
            assert got_prf == bytes([FILL]) * len(got_prf), f"{what}: proofs of skipped item {i} written"
            if nodes is not None:
                assert (nodes[i * nn * 32:(i + 1) * nn * 32] == FILL).all(), \
                    f"{what}: node slot of skipped item {i} written"
        else:
            keep[o_off[i]:o_off[i] + cnt * s] = False
            got = sym[o_off[i]:o_off[i] + cnt * s].tobytes()
            assert got == w_sym, f"{what}: symbols of item {i} {it[:3]} differ from the oracle's"
            assert got_prf == w_prf, f"{what}: proofs of item {i} {it[:3]} differ from the oracle's"
            if nodes is not None and nodes_written:
                assert nodes[i * nn * 32:(i + 1) * nn * 32].tobytes() == w_nodes, \
                    f"{what}: tree of item {i} {it[:3]} differs from the oracle's"
        j += cnt
    assert (sym[keep] == FILL).all(), f"{what}: bytes outside the accepted symbol extents were written"


def run_per_size(gpu, n, items, want_nodes=False, pool=POOL, cpu=None):
    """The same requests through rs2_verifier_recovery_symbols_multi_device_async, one call per
    (axis, size): per item (symbols, proofs, nodes or None) as bytes."""
    L, nn = shape(n)
    out = [None] * len(items)
    groups = {}
    for i, (a, s, _, _) in enumerate(items):
        groups.setdefault((a, s), []).append(i)
    for (a, s), members in groups.items():
        ref = ref_of(n, items[members[0]], cpu, pool)
        v = gpu.SliverVerifier(n, s, a)
        d_sl = to_dev(np.stack([ref["data"][items[i][2]] for i in members]))
        targets = [list(items[i][3]) for i in members]
        total = sum(len(t) for t in targets)
        d_sym = torch.full((max(total * s, 2),), FILL, dtype=torch.uint8, device=dev())
        d_prf = torch.full((max(total * L * 32, 32),), FILL, dtype=torch.uint8, device=dev())
        d_nodes = torch.full((len(members) * nn * 32,), FILL, dtype=torch.uint8, device=dev()) \
            if want_nodes else None
        assert v.recovery_symbols_multi_async(
            d_sl.data_ptr(), targets, d_sym.data_ptr(), d_prf.data_ptr(),
            d_nodes.data_ptr() if want_nodes else 0) == 0, _lib.last_error()
        torch.cuda.synchronize()
        sym, prf = d_sym.cpu().numpy(), d_prf.cpu().numpy()
        nd = d_nodes.cpu().numpy() if want_nodes else None
        j = 0
        for q, i in enumerate(members):
            cnt = len(targets[q])
            out[i] = (sym[j * s:(j + cnt) * s].tobytes(), prf[j * L * 32:(j + cnt) * L * 32].tobytes(),
                      nd[q * nn * 32:(q + 1) * nn * 32].tobytes() if want_nodes else None)
            j += cnt
    return out


def got_per_item(n, items, sym, o_off, prf, nodes=None):
    """run()'s buffers cut per item, shaped as run_per_size's result."""
    L, nn = shape(n)
    out, j = [], 0
    for i, (_, s, _, ts) in enumerate(items):
        cnt = len(ts)
        out.append((sym[o_off[i]:o_off[i] + cnt * s].tobytes(),
                    prf[j * L * 32:(j + cnt) * L * 32].tobytes(),
                    None if nodes is None else nodes[i * nn * 32:(i + 1) * nn * 32].tobytes()))
        j += cnt
    return out


def reorder(items, order):
    if order == "interleaved":
        return list(items)
    srt = sorted(items, key=lambda it: (AXES.index(it[0]), it[1], it[2]))
    return srt if order == "sorted" else srt[::-1]
