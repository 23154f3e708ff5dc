"""Structured erasure patterns for the decode tests -- TEST ONLY (a plain module, no fixtures).

The decode is the one path whose host plan and kernel control flow depend on WHICH shards are
present (rs2_planner.cpp plan_decode): the input and output blocks, each block's fill (`count`,
`trunc`, hence its active waves), the mixing kinds, the fused or separate copy of the present
originals and the P/Q block pairing all follow from the pattern.  A random k-subset at n = 1000
erases originals in every block and fills every input block to its end, so it reaches one corner
of that space.  This module supplies the rest:

  decode_layout(k, n, block_limit, present)
      the block arithmetic of plan_decode restated in Python: rate, cs0, W, C, the positions of
      originals and repairs, the input blocks with their count, the output blocks with their
      trunc, nw and the waves per block.  It does NOT restate the mixing matrices.

  families(k, n, block_limit)
      named patterns (lists of exactly k distinct shard indices), the outages a storage network
      sees -- nodes hold contiguous shard ranges, so shards go missing in bursts -- and the
      corners of the planner:
        single     one original gone (original 0, k-1, the first / last original of every
                   original block), replaced by the first or by the last repair shard
        blockout   every original of one block gone (blocks of at most r originals)
        inblock    the first / last e originals of one block gone, e = 1, half, all it can lose
        head/tail  the first / last e originals of the code gone, e = 1, half, min(k, r)
        burst      r cyclically consecutive shards gone, start every max(1, n // 16) indices and
                   centred on the original / repair seam and on the wrap-around
        comb       every 2nd / every 3rd shard gone (up to r), the first k others present
      tests/test_erasure_patterns.py proves on the CPU what these reach for each tested geometry:
      every original block as the ONLY output block, blocks that hold shards but feed no input,
      input counts of 1 and of C, trunc of 1 and of the geometry's maximum, and -- wherever a
      block spans more than one wave -- the counting precondition of the P/Q pairing (one output
      block, two input blocks whose waves fit the workgroup together) for every original block
      as the sole output, and its failure.

What cannot be shown from Python: pairing also needs M1[o][q] == 0 and M2[o][q] != 0 for some
input block q (plan_decode), a property of the mixing matrices, which live in the engine only.
Whether a given pattern takes the pair branches of load_ifft (rs2_codec.hip) is therefore not
observable here; the coverage claim is the counting precondition over every output block and
many input arrangements, and a byte-exact result for each of them.

  batch_path(lay, s), predicted_stats(lays, s), batch_jobs(fams)
      for the batched decode and recovery calls (BATCH_GEOMETRIES): the path each pattern takes
      (batched launch or per-job decode), the counters a call must add, and one call's job list
      with every family in it.

  block_limit(b)   context manager: rs2_set_block_limit(b), restored to 512 on exit.  The 1D
                   decode plans with the limit current at the call; make a fresh DeviceOps /
                   DevicePlan inside the context, never one created under another limit.
"""
import contextlib
import ctypes
from itertools import combinations

import numpy as np

import rs2_oracle as O

# (k, n, block limit) of the structured-pattern tests and the number of patterns of each
GEOMETRIES = [(34, 100, 16, 67), (67, 100, 16, 90), (100, 300, 64, 56), (200, 300, 64, 81),
              (334, 1000, 128, 69), (667, 1000, 128, 105), (334, 1000, 512, 45),
              (667, 1000, 512, 55)]
# every code that is K_p or K_s of n_shards = 4, 7, 10, with the block limits that change C
# (None = the default), 396 k-subsets in all
SMALL = [(2, 4, (None, 1)), (3, 4, (None,)), (3, 7, (None, 2, 1)), (5, 7, (None, 1)),
         (4, 10, (None, 2, 1)), (7, 10, (None, 2, 1))]
# (k, n, block limit, patterns, batch-eligible patterns at s >= 4) of the batched decode and
# recovery tests: one call carries every family of an entry, so one launch mixes n_in 1..8 with
# n_out 1..5, paired and unpaired jobs, fused and unfused ones, and -- where eligible < patterns
# -- jobs of 9 and more blocks that leave the launch for the per-job path.  (67, 100, 8) is left
# out: all its patterns have 9 or more input blocks.  tests/test_erasure_patterns.py re-derives
# the last two figures from decode_layout / batch_path.
BATCH_GEOMETRIES = [(34, 100, 16, 67, 67), (67, 100, 16, 90, 90), (34, 100, 8, 91, 90),
                    (100, 300, 64, 56, 56), (200, 300, 64, 81, 81), (200, 300, 32, 117, 102),
                    (334, 1000, 512, 45, 45), (667, 1000, 512, 55, 55), (334, 1000, 128, 69, 69),
                    (667, 1000, 128, 105, 103)]
# The same for the codes of a 300-shard BLOB: n = 300 gives K_p = 102 and K_s = 201, so the
# (100, 300) and (200, 300) codes above -- 1D codes of the decode_lines tests -- are no axis of a
# blob plan or a sliver verifier.  The planner proofs run both; the batched GPU calls, which go
# through blob plans and verifiers, run BATCH_CALLS: these at n = 300 and the entries above at
# n = 100 (K_p 34, K_s 67) and n = 1000 (K_p 334, K_s 667).
BLOB_300 = [(102, 300, 64, 57, 57), (201, 300, 64, 81, 81), (201, 300, 32, 117, 101)]
BATCH_CALLS = [g for g in BATCH_GEOMETRIES if g[1] != 300] + BLOB_300
BATCH_BLOCKS = 8      # kBatchBlocks: input / output blocks a job of a batched launch may have
CHUNK_JOBS = 341      # jobs of one planning window (an upload slot of 512 KiB / 1536-byte jobs)
DEFAULT_LIMIT = 512   # kMaxC, the engine's block limit unless lowered
PPW = 32              # kPpwTarget: positions per wave


class Layout:
    """decode_layout's result; str() is what an assertion message shows."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __str__(self):
        return (f"layout k={self.k} n={self.n} {'high' if self.high else 'low'} rate cs0={self.cs0} "
                f"W={self.W} C={self.C} blocks={self.m} nw={self.nw} "
                f"in(block,count)={self.in_blocks} out(block,trunc)={self.out_blocks} "
                f"waves={self.waves} pair_precondition={pair_precondition(self)}")


def decode_layout(k, n, block_limit, present):
    """The block arithmetic of plan_decode for the k present shard indices `present`."""
    r = n - k
    present = sorted(set(int(q) for q in present))
    assert len(present) == k and 0 <= present[0] and present[-1] < n, "need k distinct valid shards"
    high = O.use_high_rate(k, r)
    cs0 = O.next_pow2(r) if high else O.next_pow2(k)
    end = cs0 + (k if high else r)
    W = O.next_pow2(end)
    C = min(cs0, block_limit or DEFAULT_LIMIT)
    opos = [cs0 + i if high else i for i in range(k)]
    rpos = [j if high else cs0 + j for j in range(r)]
    have = set(present)
    count, trunc = {}, {}
    for q in present:
        p = opos[q] if q < k else rpos[q - k]
        count[p // C] = max(count.get(p // C, 0), p % C + 1)
    for i in range(k):
        if i not in have:
            p = opos[i]
            trunc[p // C] = max(trunc.get(p // C, 0), p % C + 1)
    ppw = min(C, PPW)
    return Layout(k=k, n=n, r=r, high=high, cs0=cs0, W=W, C=C, m=W // C, opos=opos, rpos=rpos,
                  in_blocks=sorted(count.items()), out_blocks=sorted(trunc.items()),
                  nw=max(1, C // PPW),
                  waves={b: (c + ppw - 1) // ppw for b, c in sorted(count.items())},
                  orig_blocks=sorted({p // C for p in opos}),
                  shard_blocks=sorted({p // C for p in opos + rpos}),
                  erased=[i for i in range(k) if i not in have])


def pair_precondition(lay):
    """The part of plan_decode's pairing condition that counting decides: more than one wave
    per block, exactly one output block, and two input blocks whose waves fit in nw."""
    if lay.nw <= 1 or len(lay.out_blocks) != 1:
        return False
    return any(lay.waves[p] + lay.waves[q] <= lay.nw
               for p, q in combinations([b for b, _ in lay.in_blocks], 2))


def batch_path(lay, s, may_fuse=True):
    """The path a pattern takes through a batched decode / recovery call, from its layout alone:
    "copy" when nothing is erased, "single" (the per-job decode) with 2-byte symbols, with more
    than BATCH_BLOCKS input or output blocks, or -- where the fused copy of the present originals
    is switched off (may_fuse=False, RS2_DEC_NOFUSE=1) -- with any original present; "batched"
    otherwise.  (With may_fuse the fused copy is covered for every family pattern of
    BATCH_GEOMETRIES, which tests/test_planner_batch.py proves on the planner itself.)"""
    if not lay.erased:
        return "copy"
    if s < 4 or len(lay.in_blocks) > BATCH_BLOCKS or len(lay.out_blocks) > BATCH_BLOCKS:
        return "single"
    if not may_fuse and len(lay.erased) < lay.k:
        return "single"
    return "batched"


def predicted_stats(lays, s, may_fuse=True, refused=()):
    """(launches, batched, single) a call of these layouts adds to the engine's counters: one
    launch per planning window of CHUNK_JOBS jobs that holds a batched job (the tests' tables
    stay far below the engine's per-launch table budget).  The jobs at the positions `refused`
    are invalid ones, which count nowhere.  No layout may be a plain copy."""
    paths = ["refused" if j in refused else batch_path(lay, s, may_fuse)
             for j, lay in enumerate(lays)]
    assert "copy" not in paths
    windows = sum("batched" in paths[w:w + CHUNK_JOBS] for w in range(0, len(paths), CHUNK_JOBS))
    return windows, paths.count("batched"), paths.count("single")


def batch_jobs(fams, seed=0):
    """One call's jobs from a family list: [(name, shards in the order they are handed over,
    source)].  Job j takes pattern j; its shard order is sorted on even j and seeded-shuffled on
    odd j (the recovery spec places symbols by their position in the received list, the blob plan
    by the order of the selection); its source is blob / sliver j % 4 of four distinct ones, so a
    job that wrote a neighbour's data is seen."""
    rng = np.random.default_rng(seed)
    jobs = []
    for j, (name, present) in enumerate(fams):
        sel = sorted(int(q) for q in present)
        if j % 2:
            sel = [sel[i] for i in rng.permutation(len(sel))]
        jobs.append((name, sel, j % 4))
    return jobs


def window_repeats(lays):
    """How often a family list is repeated for the two-window calls: the fewest times that give
    CHUNK_JOBS jobs of one output block, so that -- with those jobs sorted to the front -- the
    first window launches one block deep and the second as deep as the families go."""
    ones = sum(len(lay.out_blocks) == 1 for lay in lays)
    reps = -(-CHUNK_JOBS // ones)
    assert CHUNK_JOBS < reps * len(lays) <= 2 * CHUNK_JOBS
    return reps


def original_blocks(k, n, block_limit):
    """[(block, [original indices in it])] for the blocks that hold originals."""
    lay = decode_layout(k, n, block_limit, range(k))
    out = {}
    for i, p in enumerate(lay.opos):
        out.setdefault(p // lay.C, []).append(i)
    return sorted(out.items())


def max_trunc(k, n, block_limit):
    """The largest trunc the geometry allows: the deepest original position of any block."""
    lay = decode_layout(k, n, block_limit, range(k))
    return max(p % lay.C + 1 for p in lay.opos)


def families(k, n, block_limit=None):
    """[(name, present)]: every `present` is a sorted list of exactly k distinct indices < n."""
    r = n - k
    assert 0 < k < n
    blocks = original_blocks(k, n, block_limit)
    out = []

    def add(name, erased, fill):
        """Erase the originals `erased`; fill from the head or the tail of the repairs."""
        erased = sorted(set(erased))
        e = len(erased)
        assert 0 < e <= r and all(0 <= i < k for i in erased), name
        rep = range(k, k + e) if fill == "head" else range(n - e, n)
        out.append((f"{name}-fill{fill}", sorted(set(range(k)) - set(erased)) + list(rep)))

    singles = sorted({0, k - 1} | {o[0] for _, o in blocks} | {o[-1] for _, o in blocks})
    for i in singles:
        for fill in ("head", "tail"):
            add(f"single-o{i}", [i], fill)
    for b, o in blocks:
        if len(o) <= r:
            for fill in ("head", "tail"):
                add(f"blockout-b{b}", o, fill)
    for b, o in blocks:
        for e in sorted({1, max(1, len(o) // 2), min(len(o), r)}):
            add(f"inblock-b{b}-first{e}", o[:e], "head")
            add(f"inblock-b{b}-last{e}", o[-e:], "tail")
    for e in sorted({1, max(1, min(k, r) // 2), min(k, r)}):
        for fill in ("head", "tail"):
            add(f"head{e}", range(e), fill)
            add(f"tail{e}", range(k - e, k), fill)
    starts = dict.fromkeys(list(range(0, n, max(1, n // 16))) + [(k - r // 2) % n, (n - r // 2) % n])
    for a in starts:
        gone = {(a + j) % n for j in range(r)}
        out.append((f"burst-a{a}", [q for q in range(n) if q not in gone]))
    for step in (2, 3):
        gone = set(list(range(0, n, step))[:r])
        out.append((f"comb{step}", [q for q in range(n) if q not in gone][:k]))
    for name, present in out:
        assert len(present) == len(set(present)) == k and all(0 <= q < n for q in present), name
    assert len({name for name, _ in out}) == len(out)
    return out


def all_subsets(k, n):
    """Every k-subset of n shards, named by its members."""
    return [("sub" + "_".join(map(str, c)), list(c)) for c in combinations(range(n), k)]


@contextlib.contextmanager
def block_limit(b, apply=True):
    """rs2_set_block_limit(b) for the body, 512 again afterwards.  apply=False (the CPU oracle,
    to which a block limit means nothing) does nothing."""
    if not apply or b is None:
        yield
        return
    from walrus_amd import _lib
    assert _lib.lib().rs2_set_block_limit(b) == 0
    try:
        yield
    finally:
        assert _lib.lib().rs2_set_block_limit(DEFAULT_LIMIT) == 0


# ---------------------------------------------------------------------------------------------
# the shared body of the 1D pattern tests (both backends of the `ops` interface)
# ---------------------------------------------------------------------------------------------
FILL = 0xA5
TAIL = 64
BEYOND = 2 ** 64 - 1
_REF = {}


def codewords(k, n, s, lines):
    """[lines][n][s] bytes, source || repair, from the oracle's encoder; computed once per
    (k, n, s), shared and read-only."""
    key = (k, n, s)
    if key not in _REF or _REF[key].shape[0] < lines:
        rng = np.random.default_rng(k * 7919 + n * 31 + s)
        data = rng.integers(0, 256, (lines, k, s), dtype=np.uint8)
        rep = np.stack([O.rs_encode_symbols(data[i], n - k) for i in range(lines)])
        cw = np.concatenate([data, rep], axis=1)
        cw.setflags(write=False)
        _REF[key] = cw
    return _REF[key][:lines]


def cut_for(pi, lay, s):
    """The pattern's cut symbol and its limit's offset inside the symbol.  The symbol rotates
    with the pattern index: erased originals on even indices, present ones on odd (where the
    pattern has any), so both the decode store and the copy of present originals get cut."""
    k = lay.k
    have = sorted(set(range(k)) - set(lay.erased))
    pool = lay.erased if (pi % 2 == 0 and lay.erased) or not have else have
    return pool[(pi // 2 * 5) % len(pool)], 1 + 2 * (pi % (s // 2))


def run_patterns(ops, device, k, n, limit_b, s, lines, patterns):
    """Decode every pattern twice through ops.decode_lines (tight strides): with out_limit beyond
    the buffer and with one odd limit inside the last line.  The output, prefilled with FILL and
    followed by TAIL more bytes of it, must equal the source symbols below the limit and FILL at
    and past it; the source buffer must stay as it was.  Returns how many cuts fell on an erased
    and on a present original."""
    import torch
    from guarded import sync
    cw = codewords(k, n, s, lines)
    src = torch.from_numpy(cw.reshape(-1).copy()).to(device)
    before = src.clone()
    size = lines * k * s
    full = torch.cat([torch.from_numpy(cw[:, :k].reshape(-1).copy()),
                      torch.full((TAIL,), FILL, dtype=torch.uint8)]).to(device)
    fill = torch.full((size + TAIL,), FILL, dtype=torch.uint8, device=device)
    at = torch.arange(size + TAIL, device=device)
    buf = torch.empty(size + TAIL, dtype=torch.uint8, device=device)
    on_erased = on_present = 0
    for pi, (name, present) in enumerate(patterns):
        lay = decode_layout(k, n, limit_b, present)
        c, odd = cut_for(pi, lay, s)
        on_erased += c in lay.erased
        on_present += c not in lay.erased
        cut = (lines - 1) * k * s + c * s + odd
        assert cut % 2 == 1 and size - k * s < cut < size
        for limit in (BEYOND, cut):
            buf.copy_(fill)
            ops.decode_lines(k, n, s, lines, present, src, [q * s for q in present], n * s,
                             buf[:size], s, k * s, limit)
            sync(device)
            want = full if limit == BEYOND else torch.where(at < limit, full, fill)
            if not torch.equal(buf, want):
                bad = torch.nonzero(buf != want).reshape(-1)
                o = int(bad[0])
                where = ("the tail past the buffer" if o >= size else
                         f"line {o // (k * s)} symbol {o % (k * s) // s} byte {o % s} "
                         f"({'erased' if o % (k * s) // s in lay.erased else 'present'} original)")
                raise AssertionError(
                    f"{k}-of-{n} block limit {limit_b} s={s} lines={lines} pattern {name} "
                    f"out_limit={limit}: {bad.numel()} wrong byte(s), the first at offset {o}, "
                    f"{where}: got {int(buf[o])} want {int(want[o])}\n{lay}\npresent={present}")
            assert torch.equal(src, before), f"{k}-of-{n} pattern {name}: source buffer written"
    return on_erased, on_present


# ---------------------------------------------------------------------------------------------
# blobs and slivers for the blob plan's decode, from the C restatement (oracle/rs2_cpu.c)
# ---------------------------------------------------------------------------------------------
def load_cpu():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_fullsize import load_cpu as load
    return load()


def params(cpu, n, length):
    kp, ks, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    cpu.rs2cpu_params(n, length, ctypes.byref(kp), ctypes.byref(ks), ctypes.byref(s))
    return kp.value, ks.value, s.value


def odd_length(cpu, n, s):
    """An odd blob length of symbol size s that ends in the middle of the last row."""
    kp, ks, _ = params(cpu, n, 1)
    length = s * kp * ks - (ks * s) // 2
    length -= length % 2 == 0
    assert length % 2 == 1 and s * kp * ks - ks * s < length < s * kp * ks
    assert params(cpu, n, length) == (kp, ks, s)
    return length


def encode(cpu, n, length, seed):
    """(blob, primary [n][K_s*s], secondary [n][K_p*s]) from the C restatement."""
    kp, ks, s = params(cpu, n, length)
    blob = np.random.default_rng(seed).integers(0, 256, length, dtype=np.uint8)
    prim = np.empty((n, ks * s), dtype=np.uint8)
    sec = np.empty((n, kp * s), dtype=np.uint8)
    hashes, bid = np.empty(n * 64, dtype=np.uint8), np.empty(32, dtype=np.uint8)
    cpu.rs2cpu_encode(n, blob.ctypes.data, length, prim.ctypes.data, sec.ctypes.data,
                      hashes.ctypes.data, bid.ctypes.data)
    return blob, prim, sec


def check_blob(buf, want, what, lay):
    import torch
    if not torch.equal(buf, want):
        bad = torch.nonzero(buf != want).reshape(-1)
        o = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} wrong byte(s), the first at offset {o} of "
                             f"{want.numel() - 64} + 64 tail: got {int(buf[o])} want "
                             f"{int(want[o])}\n{lay}")
