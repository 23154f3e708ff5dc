"""Helpers of the mixed sliver recovery tests (tests/test_gpu_recover_mixed_*.py) -- TEST ONLY, a
plain module built on verify_mixed.py and erasure_patterns.py.  A case is a list of items
(axis, symbol size, pattern, source seed): the sliver is verify_mixed.sliver's seeded random K*s
bytes, expanded once per (n, size, axis, seed) by the oracle's 1D encode (shared, read-only); its
received symbols are the pattern's shards in the handed-over order; its reference root is
verify_mixed.root -- the Python oracle below n = 100, the C restatement from there on.  `run`
issues one rs2_sliver_checker_recover_device_async call on torch buffers and returns what it
wrote; `predicted` restates the windows and the range cut in Python from decode_layout and
batch_path alone."""
import ctypes

import numpy as np
import torch

import erasure_patterns as EP
import rs2_oracle as O
import verify_mixed as M
from walrus_amd import _lib

AXES = M.AXES
SIZES = [4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258]   # 256: one tile of 64 element pairs
SIZES_1000 = [20, 66, 130, 1206]
FILL = 0xEE
MATCH, MISMATCH, SKIPPED = M.MATCH, M.MISMATCH, M.SKIPPED
WINDOW_GROUPS = 256            # RS2_VERIFY_MIXED_WINDOW_GROUPS
WINDOW_SLIVERS = EP.CHUNK_JOBS  # jobs of one upload slot

k_of = M.k_of
_CW = {}


def codeword(n, s, axis, seed=0):
    """[n][s]: the sliver's K symbols and the oracle's n - K repair symbols."""
    key = (n, s, axis, seed)
    if key not in _CW:
        k = k_of(n, axis)
        data = M.sliver(n, s, axis, seed).reshape(k, s)
        cw = np.concatenate([data, O.rs_encode_symbols(data, n - k)], axis=0)
        cw.setflags(write=False)
        _CW[key] = cw
    return _CW[key]


def handed_over(present, j, seed=0):
    """The shard order of item j: sorted on even j, seeded-shuffled on odd j (the recovery spec
    places symbols by their position in the received list)."""
    sel = sorted(int(q) for q in present)
    if j % 2:
        rng = np.random.default_rng([seed, j])
        sel = [sel[i] for i in rng.permutation(len(sel))]
    return sel


def family_case(n, sizes, limit=None, repeat=1, only_batched=True):
    """Every family pattern of both axes at block limit `limit`, the sizes cycling through them
    (axis a's pattern j has size sizes[(j + a) % len]), primary and secondary items alternating
    while both last.  only_batched drops the patterns batch_path sends elsewhere."""
    per_axis = []
    for ai, axis in enumerate(AXES):
        k = k_of(n, axis)
        fams = EP.families(k, n, limit) * repeat
        items = []
        for j, (_, present) in enumerate(fams):
            s = sizes[(j + ai) % len(sizes)]
            if only_batched and EP.batch_path(EP.decode_layout(k, n, limit, present), s) != "batched":
                continue
            items.append((axis, s, handed_over(present, j), j % M.POOL))
        per_axis.append(items)
    out = []
    for j in range(max(len(x) for x in per_axis)):
        out += [x[j] for x in per_axis if j < len(x)]
    return out


def reorder(items, order):
    if order == "interleaved":
        return list(items)
    srt = sorted(items, key=lambda it: (AXES.index(it[0]), it[1]))
    return srt if order == "sorted" else srt[::-1]


def layout(n, items, gap=6):
    """(symbol offsets, symbol buffer size, output offsets, output size): sliver i's received
    symbols back to back, 2 bytes between neighbours' runs; `gap` bytes between output slivers."""
    s_off, o_off, sa, oa = [], [], 0, 0
    for a, s, pat, _ in items:
        s_off.append(sa)
        o_off.append(oa)
        sa += len(pat) * s + 2
        oa += k_of(n, a) * s + gap
    return s_off, max(sa - 2, 2), o_off, max(oa - gap, 2)


def received(n, item):
    """The item's received symbols back to back, in the handed-over order."""
    a, s, pat, seed = item
    return codeword(n, s, a, seed)[pat].reshape(-1)


def payload(n, items, s_off, size, data=None):
    buf = np.full(size, 0x5A, dtype=np.uint8)
    for i, it in enumerate(items):
        d = received(n, it) if data is None or data[i] is None else \
            np.frombuffer(bytes(data[i]), dtype=np.uint8)
        buf[s_off[i]:s_off[i] + d.size] = d
    return buf


def want_sliver(n, item):
    a, s, _, seed = item
    return M.sliver(n, s, a, seed).tobytes()


def expected_roots(n, items):
    return b"".join(M.root(n, s, a, seed) for a, s, _, seed in items)


def stats():
    out = (ctypes.c_uint64 * 5)()
    assert _lib.lib().rs2_recover_mixed_stats(out) == 0
    return [int(x) for x in out]


def moved(before):
    return [a - b for a, b in zip(stats(), before)]


def recover_stats():
    out = (ctypes.c_uint64 * 3)()
    assert _lib.lib().rs2_recover_stats(out) == 0
    return [int(x) for x in out]


def windows(n, items, budget, accepted=None):
    """The window rule restated: lists of item indices.  Slivers are taken in order; a window
    closes before the sliver that takes its scratch past the budget, opens group 257 or is its
    342nd accepted sliver; it always holds one."""
    out, cur, used, groups = [], [], 0, set()
    for i, (a, s, _, _) in enumerate(items):
        if accepted is not None and not accepted[i]:
            continue
        need = M.scratch(n, s)
        if cur and (used + need > budget or len(cur) >= WINDOW_SLIVERS or
                    ((a, s) not in groups and len(groups) == WINDOW_GROUPS)):
            out.append(cur)
            cur, used, groups = [], 0, set()
        cur.append(i)
        used += need
        groups.add((a, s))
    out.append(cur)
    return out


def predicted(n, items, budget, limit=None, accepted=None):
    """[windows, range launches, slivers inside them, per-sliver decodes, groups] a call adds:
    per window one range launch per block size C among its batched slivers (the tests' tables
    stay far below the per-launch table budget), the "single" and "copy" paths per sliver."""
    wins = windows(n, items, budget, accepted)
    launches = batched = single = groups = 0
    for win in wins:
        classes = set()
        for i in win:
            a, s, pat, _ = items[i]
            lay = EP.decode_layout(k_of(n, a), n, limit, pat)
            if EP.batch_path(lay, s) == "batched":
                classes.add(lay.C)
                batched += 1
            else:
                single += 1
        launches += len(classes)
        groups += len({(items[i][0], items[i][1]) for i in win})
    return [len(wins), launches, batched, single, groups]


def dev():
    return M.dev()


def run(checker, n, items, expected=None, statuses=False, data=None, gap=6, stream=None,
        want_roots=True, index_lists=None):
    """One call over `items`.  Returns (rc or statuses, output buffer as numpy, output offsets,
    roots bytes, verdict list or None) after a device synchronize; outputs start as FILL.
    data: received bytes per item that replace the oracle's; index_lists: the symbol indices
    handed over, when they are not the items' patterns."""
    m = len(items)
    s_off, s_size, o_off, o_size = layout(n, items, gap)
    d_sym = torch.tensor(payload(n, items, s_off, s_size, data), dtype=torch.uint8, device=dev())
    before = d_sym.clone()
    d_out = torch.full((o_size,), FILL, dtype=torch.uint8, device=dev())
    d_roots = torch.full((max(m, 1) * 32,), FILL, dtype=torch.uint8, device=dev())
    d_verdict = torch.full((max(m, 1) * 4,), FILL, dtype=torch.uint8, device=dev()) \
        if expected is not None else None
    torch.cuda.synchronize()
    res = checker.recover_async(
        [a for a, _, _, _ in items], [s for _, s, _, _ in items],
        index_lists if index_lists is not None else [p for _, _, p, _ in items],
        d_sym.data_ptr(), s_off, d_out.data_ptr(), o_off, expected,
        d_roots.data_ptr() if want_roots else 0,
        d_verdict.data_ptr() if d_verdict is not None else 0, stream, statuses)
    torch.cuda.synchronize()
    assert torch.equal(d_sym, before), "the symbol buffer was written"
    verdict = None
    if d_verdict is not None:
        verdict = d_verdict.cpu().numpy().view(np.int32)[:m].tolist()
    return res, d_out.cpu().numpy(), o_off, d_roots.cpu().numpy().tobytes()[:m * 32], verdict


def check_slivers(n, items, out, o_off, gap=6, want=None, skipped=(), what=""):
    """Every accepted sliver equals the oracle's (want[i] replaces it), every skipped one's extent
    and every gap still hold FILL."""
    keep = np.ones(out.size, dtype=bool)
    for i, it in enumerate(items):
        ln = k_of(n, it[0]) * it[1]
        if i in skipped:
            continue
        keep[o_off[i]:o_off[i] + ln] = False
        w = want_sliver(n, it) if want is None or want[i] is None else bytes(want[i])
        got = out[o_off[i]:o_off[i] + ln].tobytes()
        if got != w:
            bad = [b for b in range(ln) if got[b] != w[b]]
            raise AssertionError(
                f"{what}: sliver {i} {it[0]} s={it[1]} seed {it[3]}: {len(bad)} wrong byte(s), the "
                f"first at byte {bad[0]} (symbol {bad[0] // it[1]}): got {got[bad[0]]} want "
                f"{w[bad[0]]}\n{EP.decode_layout(k_of(n, it[0]), n, None, it[2])}")
    assert (out[keep] == FILL).all(), f"{what}: bytes outside the accepted slivers were written"


def check_roots(n, items, got, skipped=(), what=""):
    want = expected_roots(n, items)
    for i in range(len(items)):
        g = got[32 * i:32 * i + 32]
        if i in skipped:
            assert g == bytes([FILL]) * 32, f"{what}: root slot of skipped sliver {i} written"
        else:
            assert g == want[32 * i:32 * i + 32], \
                f"{what}: root {i} {items[i][:2]} differs from the oracle's"
