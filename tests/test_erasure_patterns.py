"""CPU self-test of tests/erasure_patterns.py: the planner arithmetic restated there, and what
the pattern families reach in each geometry the device tests run (no GPU, no engine)."""
import pytest

from erasure_patterns import (BATCH_BLOCKS, BATCH_CALLS, BATCH_GEOMETRIES, BLOB_300, CHUNK_JOBS,
                              GEOMETRIES, SMALL,
                              all_subsets, batch_jobs, batch_path, cut_for, decode_layout, families,
                              max_trunc, original_blocks, pair_precondition, predicted_stats, window_repeats)


def test_layout_restates_the_planner():
    """Hand-checked values of plan_decode's arithmetic."""
    lay = decode_layout(667, 1000, None, range(333, 1000))      # "the last K shards"
    assert (lay.high, lay.cs0, lay.W, lay.C, lay.m, lay.nw) == (True, 512, 2048, 512, 4, 16)
    assert lay.opos[0] == 512 and lay.rpos[0] == 0
    # originals 0..332 erased: all in block 1; present: originals 333..666 (positions 845..1178,
    # blocks 1 and 2) and every repair (block 0, positions 0..332)
    assert lay.out_blocks == [(1, 333)]
    assert lay.in_blocks == [(0, 333), (1, 512), (2, 155)]
    assert lay.waves == {0: 11, 1: 16, 2: 5} and pair_precondition(lay)
    lay = decode_layout(334, 1000, 128, list(range(1, 334)) + [999])
    assert (lay.high, lay.cs0, lay.W, lay.C, lay.m, lay.nw) == (False, 512, 2048, 128, 16, 4)
    assert lay.opos[333] == 333 and lay.rpos[665] == 512 + 665
    assert lay.out_blocks == [(0, 1)]                           # original 0 at position 0
    assert lay.in_blocks == [(0, 128), (1, 128), (2, 78), (9, 26)]   # 1177 = 9 * 128 + 25
    assert lay.waves == {0: 4, 1: 4, 2: 3, 9: 1} and pair_precondition(lay)
    lay = decode_layout(7, 10, 1, [0, 1, 2, 3, 4, 5, 9])
    assert (lay.high, lay.cs0, lay.W, lay.C, lay.m, lay.nw) == (True, 4, 16, 1, 16, 1)
    assert lay.out_blocks == [(10, 1)] and lay.in_blocks == [(b, 1) for b in (2, 4, 5, 6, 7, 8, 9)]
    assert not pair_precondition(lay)
    assert decode_layout(2, 4, None, [0, 1]).out_blocks == []   # all sources present
    with pytest.raises(AssertionError):
        decode_layout(3, 7, None, [0, 1, 1])


@pytest.mark.parametrize("k,n,limit,count", GEOMETRIES)
def test_families_reach_the_planner_corners(k, n, limit, count):
    fams = families(k, n, limit)
    assert len(fams) == count
    lays = [decode_layout(k, n, limit, present) for _, present in fams]
    C, nw = lays[0].C, lays[0].nw
    assert C == limit
    sole = {lay.out_blocks[0][0] for lay in lays if len(lay.out_blocks) == 1}
    orig = [b for b, _ in original_blocks(k, n, limit)]
    assert sole == set(orig)                                                        # (a)
    assert any(set(lay.shard_blocks) - {b for b, _ in lay.in_blocks} for lay in lays)   # (b)
    counts = {c for lay in lays for _, c in lay.in_blocks}
    assert {1, C} <= counts                                                         # (c)
    truncs = {t for lay in lays for _, t in lay.out_blocks}
    assert {1, max_trunc(k, n, limit)} <= truncs                                    # (d)
    if nw > 1:                                                                      # (e)
        paired = {lay.out_blocks[0][0] for lay in lays if pair_precondition(lay)}
        assert paired == set(orig)
        # and it fails, also for a single output block (too few or too full input blocks)
        assert any(len(lay.out_blocks) == 1 and not pair_precondition(lay) for lay in lays)
    else:
        assert not any(pair_precondition(lay) for lay in lays)
    # every pattern loses an original (else nothing is decoded) and is decodable (k shards)
    assert all(lay.erased and len(lay.erased) <= n - k for lay in lays)


# What the one call of each BATCH_GEOMETRIES entry holds: the n_in and the n_out values of its
# jobs (input / output blocks, ineligible jobs included).
BATCH_REACH = {
    (34, 100, 16): ({3, 4, 5, 6}, {1, 2, 3}),
    (67, 100, 16): ({5, 6, 7, 8}, {1, 2, 3, 5}),
    (34, 100, 8): ({5, 6, 7, 8, 10}, {1, 2, 3, 4, 5}),
    (100, 300, 64): ({2, 3, 4}, {1, 2}),
    (200, 300, 64): ({4, 5, 6}, {1, 2, 3, 4}),
    (200, 300, 32): ({7, 8, 9, 11}, {1, 2, 3, 4, 7}),
    (334, 1000, 512): ({1, 2, 3}, {1}),
    (667, 1000, 512): ({2, 3}, {1, 2}),
    (334, 1000, 128): ({3, 4, 5, 6}, {1, 2, 3}),
    (667, 1000, 128): ({6, 7, 9}, {1, 2, 3, 4, 6}),
    # the codes of a 300-shard blob reach what (100, 300) and (200, 300) reach
    (102, 300, 64): ({2, 3, 4}, {1, 2}),
    (201, 300, 64): ({4, 5, 6}, {1, 2, 3, 4}),
    (201, 300, 32): ({7, 8, 9, 11}, {1, 2, 3, 4, 7}),
}
# the entries whose call must mix at least three launch depths (grid.z against a job's n_out)
THREE_N_OUT = {(34, 100, 16), (67, 100, 16), (34, 100, 8), (200, 300, 64), (200, 300, 32),
               (334, 1000, 128), (667, 1000, 128), (201, 300, 64), (201, 300, 32)}
# the entries with per-job decodes between batched jobs
WITH_FALLBACKS = {(200, 300, 32), (667, 1000, 128), (201, 300, 32)}


def test_batch_calls_are_codes_of_a_blob():
    """Every BATCH_CALLS entry is K_p or K_s of its n (so a blob plan and a sliver verifier can
    run it), both axes of n = 100, 300 and 1000 occur, and only the n = 300 entries of
    BATCH_GEOMETRIES had to be replaced."""
    import rs2_oracle as O
    assert {(n, O.source_symbols_for_n_shards(n).index(k)) for k, n, _, _, _ in BATCH_CALLS} == \
        {(n, axis) for n in (100, 300, 1000) for axis in (0, 1)}
    assert O.source_symbols_for_n_shards(300) == (102, 201)
    assert [g for g in BATCH_GEOMETRIES if g not in BATCH_CALLS] == \
        [g for g in BATCH_GEOMETRIES if g[1] == 300]
    assert [(round(k, -2), n, limit) for k, n, limit, _, _ in BLOB_300] == \
        [(k, n, limit) for k, n, limit, _, _ in BATCH_GEOMETRIES if n == 300]   # limit for limit


@pytest.mark.parametrize("k,n,limit,count,eligible", BATCH_GEOMETRIES + BLOB_300)
def test_batch_calls_are_heterogeneous(k, n, limit, count, eligible):
    """What keeps the batched GPU tests (test_gpu_patterns_3_batch / _4_recover) from passing
    vacuously, from the reference arithmetic alone: one call of a geometry holds jobs of several
    n_in and n_out, paired and unpaired ones, ones with and without a present original, and --
    where some patterns have more than 8 blocks -- per-job decodes between batched jobs."""
    fams = families(k, n, limit)
    assert len(fams) == count
    assert [name for name, _, _ in batch_jobs(fams)] == [name for name, _ in fams]
    lays = [decode_layout(k, n, limit, present) for _, present in fams]
    for s in (6, 66, 130):
        paths = [batch_path(lay, s) for lay in lays]
        assert set(paths) <= {"batched", "single"}      # no family pattern is a plain copy
        assert paths.count("batched") == eligible
        assert predicted_stats(lays, s) == (1, eligible, count - eligible)
    assert {batch_path(lay, 2) for lay in lays} == {"single"}
    shape = [(len(lay.in_blocks), len(lay.out_blocks)) for lay in lays]
    n_in, n_out = BATCH_REACH[k, n, limit]
    assert {a for a, _ in shape} == n_in and {b for _, b in shape} == n_out
    assert ((k, n, limit) in THREE_N_OUT) == (len(n_out) >= 3)
    # the eligibility rule restated: at most 8 blocks either way
    assert [p == "batched" for p in paths] == [max(a, b) <= BATCH_BLOCKS for a, b in shape]
    if (k, n, limit) == (67, 100, 16):
        assert (8, 5) in shape                                        # the 8-block edge
    switches = sum(paths[j] != paths[j + 1] for j in range(count - 1))
    if (k, n, limit) in WITH_FALLBACKS:
        assert eligible < count and switches >= 1   # a per-job decode between batched jobs
    else:
        assert count - eligible <= 1
    paired = [pair_precondition(lay) for lay in lays]
    if lays[0].C >= 64:
        assert any(paired) and not all(paired)
    else:
        assert not any(paired)
    # with and without a present original.  A pattern keeps k of n shards, so at least
    # k - (n - k) originals are present: only a low-rate code (k <= n - k) can lose them all.
    originals = [k - len(lay.erased) for lay in lays]
    assert any(originals)
    if k <= n - k:
        assert 0 in originals
    else:
        assert min(originals) >= 2 * k - n > 0
    # RS2_DEC_NOFUSE=1: every job with a present original leaves the batch
    nofuse = predicted_stats(lays, 6, may_fuse=False)
    assert nofuse[1] == sum(o == 0 and p == "batched" for o, p in zip(originals, paths))
    assert nofuse[1] + nofuse[2] == count and nofuse[0] == (nofuse[1] > 0)


@pytest.mark.parametrize("k,n,limit,reps", [(34, 100, 16, 9), (67, 100, 16, 6)])
def test_batch_jobs_order_sources_and_windows(k, n, limit, reps):
    fams = families(k, n, limit)
    assert window_repeats([decode_layout(k, n, limit, p) for _, p in fams]) == reps
    jobs = batch_jobs(fams * reps)
    assert CHUNK_JOBS < len(jobs) == reps * len(fams) <= 2 * CHUNK_JOBS
    for j, ((name, sel, src), (fname, present)) in enumerate(zip(jobs, fams * reps)):
        assert name == fname and sorted(sel) == sorted(present) and src == j % 4
        assert (sel == sorted(sel)) == (j % 2 == 0)
    assert batch_jobs(fams) == jobs[:len(fams)] and batch_jobs(fams, seed=1) != jobs[:len(fams)]
    # a pattern meets more than one source over the repeats
    assert len({src for name, _, src in jobs if name == fams[1][0]}) > 1
    # two planning windows; with the one-block jobs first, each has its own largest n_out
    lays = [decode_layout(k, n, limit, sel) for _, sel, _ in jobs]
    assert predicted_stats(lays, 6) == (2, len(jobs), 0)
    depth = sorted((len(lay.out_blocks) for lay in lays), key=lambda d: d != 1)
    assert max(depth[:CHUNK_JOBS]) == 1 < max(depth[CHUNK_JOBS:])
    assert max(len(lay.out_blocks) for lay in lays[:CHUNK_JOBS]) > 1   # family order: both deep


@pytest.mark.parametrize("k,n,limit,count", GEOMETRIES)
def test_cuts_rotate_over_erased_and_present(k, n, limit, count):
    for s in (2, 6, 66):
        hit = set()
        for pi, (_, present) in enumerate(families(k, n, limit)):
            lay = decode_layout(k, n, limit, present)
            c, odd = cut_for(pi, lay, s)
            assert 0 <= c < k and odd % 2 == 1 and odd < s
            hit.add((c in lay.erased, c))
        assert len({c for e, c in hit if e}) > 3 and len({c for e, c in hit if not e}) > 3


def test_small_codes_are_exhaustive():
    total = 0
    for k, n, limits in SMALL:
        subs = all_subsets(k, n)
        total += len(subs)
        assert len({tuple(p) for _, p in subs}) == len(subs)
        cs = [decode_layout(k, n, b, range(k)).C for b in limits]
        assert len(set(cs)) == len(cs) and cs[0] == decode_layout(k, n, 512, range(k)).C
        assert set(cs) == {c for c in (1, 2, 4) if c <= cs[0]}   # every limit that changes C
    assert total == 396
    assert decode_layout(7, 10, 1, range(7)).m == 16            # 16 blocks of one position


@pytest.mark.parametrize("fault", ["none", "wrong_byte", "past_limit", "tail", "source", "skipped"])
def test_the_shared_body_notices(fault):
    """run_patterns itself, on the oracle backend with a fault put in: one wrong byte in a
    decoded symbol, a write at the limit, a write past the buffer, a write to the source, and
    an erased symbol left unwritten must each fail it."""
    import torch
    from cpu_ops import CpuOps
    from erasure_patterns import BEYOND, run_patterns
    k, n, s, lines = 3, 7, 6, 2

    class Faulty(CpuOps):
        def decode_lines(self, k_, n_, s_, lines_, idx, base, sym_off, ls, out, oss, ols, limit):
            erased = [i for i in range(k_) if i not in idx]
            keep = out.clone()
            super().decode_lines(k_, n_, s_, lines_, idx, base, sym_off, ls, out, oss, ols, limit)
            full = out.data_ptr() + out.numel()   # the buffer behind the view handed in
            if fault == "wrong_byte" and limit == BEYOND:
                out[ols + erased[0] * oss + 1] ^= 0x10
            elif fault == "past_limit" and limit != BEYOND:
                out[limit] = 0
            elif fault == "tail":
                import ctypes
                ctypes.memset(full + 5, 0, 1)
            elif fault == "source":
                base[3] ^= 1
            elif fault == "skipped" and limit == BEYOND:
                o = erased[-1] * oss
                out[o:o + s_] = keep[o:o + s_]

    subs = [p for p in all_subsets(k, n) if len(set(range(k)) - set(p[1]))]

    def run():
        return run_patterns(Faulty(), torch.device("cpu"), k, n, None, s, lines, subs)

    if fault == "none":
        assert all(run())
    else:
        with pytest.raises(AssertionError, match="wrong byte|source buffer written"):
            run()
