"""Bulk sliver recovery (SliverVerifier.recover_slivers_async) under the structured erasure
patterns.

One call recovers a sliver from EVERY family pattern of a geometry
(erasure_patterns.BATCH_CALLS): sliver j is sliver j % 4 of four oracle slivers, recovered
from family j's symbols, handed over in sorted (even j) or shuffled (odd j) order.  The 1D
decodes share one launch per window although their block counts, pairing and fused copies differ
(tests/test_erasure_patterns.py proves the mix on the CPU), and the slivers of more than 8 blocks
take the per-sliver decode between them, which leaves a gap in the chunk but none in the root and
verdict runs.  Expected roots are given; outputs, roots, verdicts, guard bands, the received
symbols and the rs2_recover_stats deltas are compared exactly with the oracle and with what
erasure_patterns.batch_path predicts from the layout alone.
"""
import numpy as np
import pytest

import rs2_oracle as O
from erasure_patterns import (BATCH_CALLS, CHUNK_JOBS, batch_jobs, batch_path, block_limit,
                              decode_layout, families, predicted_stats, window_repeats)
from test_gpu_recover_batch import (MATCH, MISMATCH, OK, E_UNSUCCESSFUL, Call, Sliver,
                                    _check_exact, _stats)

pytestmark = pytest.mark.gpu

_SLIVERS = {}


def slivers_for(k, n, s):
    """Four oracle slivers of k symbols of an n-shard code; shared and read-only."""
    if (k, n, s) not in _SLIVERS:
        rng = np.random.default_rng(k * 7919 + n * 31 + s)
        _SLIVERS[k, n, s] = [Sliver(n, k, s, rng) for _ in range(4)]
        assert len({sl.root for sl in _SLIVERS[k, n, s]}) == 4
    return _SLIVERS[k, n, s]


def axis_of(k, n):
    """A primary sliver has K_s symbols, a secondary one K_p."""
    kp, ks = O.source_symbols_for_n_shards(n)
    assert k in (kp, ks)
    return "primary" if k == ks else "secondary"


class FamilyCall:
    """The call of a family list: job j recovers sliver j % 4 from pattern j's symbols.
    `lists` / `datas` may be edited before run()."""

    def __init__(self, k, n, limit, s, fams):
        self.k, self.n, self.limit, self.s = k, n, limit, s
        self.axis = axis_of(k, n)
        self.jobs = batch_jobs(fams)
        base = slivers_for(k, n, s)
        self.slivers = [base[src] for _, _, src in self.jobs]
        self.lays = [decode_layout(k, n, limit, sel) for _, sel, _ in self.jobs]
        self.lists = [list(sel) for _, sel, _ in self.jobs]
        self.datas = [sl.all[sel].copy() for sl, sel in zip(self.slivers, self.lists)]
        self.expected = [sl.root for sl in self.slivers]
        self.what = f"{k}-of-{n} block limit {limit} s={s} {self.axis}"

    def run(self, statuses=False, refused=(), may_fuse=True):
        """Issue the call with a verifier of its own; (call, stats delta, predicted, codes)."""
        from walrus_amd.encoding import SliverVerifier
        call = Call(self.n, self.s, self.axis, self.lists, self.datas, self.expected)
        assert call.K == self.k
        with block_limit(self.limit):
            v = SliverVerifier(self.n, self.s, self.axis)
            before = _stats()
            codes = call.run(v, statuses=statuses)
            call.results()   # synchronises
            delta = (_stats() - before).tolist()
            del v
        predicted = predicted_stats(self.lays, self.s, may_fuse, set(refused))
        return call, delta, predicted, codes

    def describe(self, j):
        return (f"{self.what}: sliver {j} (pattern {self.jobs[j][0]}, "
                f"{batch_path(self.lays[j], self.s)})\n{self.lays[j]}")


def check_exact(fc, call, skipped=()):
    try:
        _check_exact(call, fc.slivers, skipped)
    except AssertionError:
        out, roots, verdict = call.results()
        for j, sl in enumerate(fc.slivers):   # name the first job that is off
            if j not in skipped and not (np.array_equal(out[j], sl.data.reshape(-1)) and
                                         roots[j].tobytes() == sl.root and verdict[j] == MATCH):
                raise AssertionError(fc.describe(j))
        raise


def sizes_for(n):
    return (6, 66) if n == 100 else (6,)


CASES = [(k, n, limit) for k, n, limit, _, _ in BATCH_CALLS] + \
    [(334, 1000, 256), (667, 1000, 256)]


# ---- 1. one call per geometry -------------------------------------------------------------------
@pytest.mark.parametrize("k,n,limit,s", [
    pytest.param(k, n, limit, s, id=f"{k}of{n}-C{limit}-s{s}")
    for k, n, limit in CASES for s in sizes_for(n)])
def test_families_one_call(gpu, k, n, limit, s):
    fams = families(k, n, limit)
    fc = FamilyCall(k, n, limit, s, fams)
    call, delta, predicted, rc = fc.run()
    print(f"{fc.what}: {len(fams)} slivers, (launches, batched, single) = {delta}")
    assert rc == OK
    check_exact(fc, call)
    assert delta == list(predicted), (fc.what, delta, predicted)
    for kk, nn, ll, count, eligible in BATCH_CALLS:
        if (kk, nn, ll) == (k, n, limit):
            assert predicted == (1, eligible, count - eligible)


# ---- 2. verdicts under heterogeneity ---------------------------------------------------------------
@pytest.mark.parametrize("k,n,limit", [(201, 300, 32), (667, 1000, 128)])
def test_verdicts_between_batched_and_fallback_jobs(gpu, k, n, limit):
    """Every 7th sliver is given the next sliver's expected root, every 11th has one bit of one
    received symbol flipped (a present original and a repair symbol in turn): MISMATCH exactly
    there.  A flipped sliver's output and root are those of the oracle's decode of the symbols as
    received: a flipped original shows flipped, and -- a reconstructed symbol depends on every
    received one -- the erased symbols change with it; a flipped repair symbol changes erased
    symbols only.  Every other sliver of the call is exact."""
    s = 6
    fc = FamilyCall(k, n, limit, s, families(k, n, limit))
    m = len(fc.jobs)
    swapped = set(range(6, m, 7))
    for j in swapped:
        fc.expected[j] = slivers_for(k, n, s)[(j + 1) % 4].root   # job j + 1's sliver
        assert fc.expected[j] != fc.slivers[j].root
    flipped = {}
    for c, j in enumerate(range(10, m, 11)):
        sel = fc.lists[j]
        pos = [p for p, q in enumerate(sel) if (q < k) == (c % 2 == 0)]
        p = pos[(3 * c) % len(pos)]
        fc.datas[j][p, c % s] ^= 1 << (c % 8)
        flipped[j] = (sel[p], c % s, 1 << (c % 8))
    assert {q < k for q, _, _ in flipped.values()} == {True, False}
    call, delta, predicted, rc = fc.run()
    assert rc == OK
    out, roots, verdict = call.results()
    for j, sl in enumerate(fc.slivers):
        want = sl.data
        if j in flipped:
            # the oracle's decode of what was received: the sliver that is consistent with it
            q, byte, bit = flipped[j]
            want = O.rs_decode_symbols(k, n, s, list(zip(fc.lists[j], fc.datas[j])))
            off = np.nonzero((want != sl.data).any(axis=1))[0].tolist()
            if q < k:   # the flipped original itself, and with it the reconstructed ones
                assert want[q, byte] == sl.data[q, byte] ^ bit and q in off, fc.describe(j)
                assert set(off) - {q} <= set(fc.lays[j].erased), fc.describe(j)
            else:
                assert off and set(off) <= set(fc.lays[j].erased), fc.describe(j)
            assert np.array_equal(out[j], want.reshape(-1)), fc.describe(j)
            assert roots[j].tobytes() == O.merkle_root(
                [x.tobytes() for x in O.rs_encode_all(want, n)]) != sl.root, fc.describe(j)
            assert verdict[j] == MISMATCH, fc.describe(j)
            continue
        assert np.array_equal(out[j], want.reshape(-1)), fc.describe(j)
        assert roots[j].tobytes() == sl.root, fc.describe(j)
        assert verdict[j] == (MISMATCH if j in swapped else MATCH), fc.describe(j)
    call.assert_guards()
    assert delta == list(predicted) and predicted[2] > 0, (fc.what, delta, predicted)


# ---- 3. surplus and duplicate symbols ----------------------------------------------------------------
@pytest.mark.parametrize("k,n,limit", [(34, 100, 8), (201, 300, 32), (334, 1000, 512)])
def test_surplus_and_duplicates_keep_the_pattern(gpu, k, n, limit):
    """Every 5th list gets a duplicate of its first symbol in front and one surplus valid symbol
    at the end: the first k distinct indices are still the family pattern (rs2_planner.cpp
    select_recovery_symbols), so the counters and every output are as without them."""
    s = 6
    fc = FamilyCall(k, n, limit, s, families(k, n, limit))
    for j in range(4, len(fc.jobs), 5):
        sel, sl = fc.lists[j], fc.slivers[j]
        spare = next(q for q in range(n - 1, -1, -1) if q not in sel)
        fc.lists[j] = [sel[0]] + sel + [spare]
        fc.datas[j] = sl.all[fc.lists[j]].copy()
        assert len(fc.lists[j]) == k + 2
    call, delta, predicted, rc = fc.run()
    assert rc == OK
    check_exact(fc, call)
    assert delta == list(predicted), (fc.what, delta, predicted)


# ---- 4. two windows ------------------------------------------------------------------------------------
def test_two_windows_with_refused_slots(gpu):
    """(67, 100, 16) repeated to more than 341 slivers: roots and verdicts of every slot of both
    windows; a refused slot (one symbol short) is SKIPPED, its output and root untouched."""
    k, n, limit, s = 67, 100, 16, 6
    fams = families(k, n, limit)
    fams = fams * window_repeats([decode_layout(k, n, limit, p) for _, p in fams])
    fc = FamilyCall(k, n, limit, s, fams)
    m = len(fc.jobs)
    assert CHUNK_JOBS < m <= 2 * CHUNK_JOBS
    refused = (7, CHUNK_JOBS - 1, CHUNK_JOBS, m - 1)
    for j in refused:
        fc.lists[j] = fc.lists[j][:-1]
        fc.datas[j] = fc.datas[j][:-1]
    call, delta, predicted, codes = fc.run(statuses=True, refused=refused)
    assert codes == [E_UNSUCCESSFUL if j in refused else OK for j in range(m)]
    check_exact(fc, call, skipped=refused)
    assert predicted == (2, m - len(refused), 0)
    assert delta == list(predicted), (fc.what, delta, predicted)
