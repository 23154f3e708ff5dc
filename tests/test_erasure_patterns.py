"""CPU self-test of tests/erasure_patterns.py: the planner arithmetic restated there, and what
the pattern families reach in each geometry the device tests run (no GPU, no engine)."""
import pytest

from erasure_patterns import (GEOMETRIES, SMALL, all_subsets, cut_for, decode_layout, families,
                              max_trunc, original_blocks, pair_precondition)


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
