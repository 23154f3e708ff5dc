"""rs2_sliver_checker_recover_device_async against the oracle: slivers of both axes and many
symbol sizes in one call, each recovered from a structured erasure pattern
(erasure_patterns.families).  Outputs, roots and MATCH verdicts are exact; the counters move by
what recover_mixed.predicted computes from decode_layout, batch_path and a Python restatement of
the windows and the range cut -- one range launch per block size per window and, in the main
cases, nothing on the per-sliver path: a sliver that falls off the batched path fails the test.

Sizes: 256 bytes is exactly one tile of 64 element pairs, 258 makes a sliver's range two tiles,
254 has 64 pairs with the last one half filled -- where the range search and tile - tile_first go
wrong.  rs2_recover_stats is pinned: the mixed call does not touch it."""
import numpy as np
import pytest
import torch

import erasure_patterns as EP
import recover_mixed as R
import verify_mixed as M
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 256 << 20


def _check(checker, n, items, budget, limit=None, what=""):
    want = R.expected_roots(n, items)
    M.set_budget(budget)
    try:
        before, before_rec, before_vm = R.stats(), R.recover_stats(), M.stats()
        rc, out, o_off, roots, verdict = R.run(checker, n, items, expected=want)
        moved, vm = R.moved(before), M.moved(before_vm)
    finally:
        M.set_budget(0)
    assert rc == 0, (rc, _lib.last_error())
    R.check_slivers(n, items, out, o_off, what=what)
    R.check_roots(n, items, roots, what=what)
    assert verdict == [R.MATCH] * len(items), what
    assert moved == R.predicted(n, items, budget, limit), what
    assert R.recover_stats() == before_rec, "rs2_recover_stats moved"
    # the verification half counts as a mixed verification of the same windows would
    assert vm[0] == moved[0] and vm[1] + vm[2] == len(items) and vm[3] == moved[4], what
    return moved


@pytest.mark.parametrize("order", ["interleaved", "sorted", "reverse"])
@pytest.mark.parametrize("n", [10, 13, 100])
def test_families_both_axes(gpu, n, order):
    items = R.reorder(R.family_case(n, R.SIZES), order)
    assert {(a, s) for a, s, _, _ in items} == {(a, s) for a in R.AXES for s in R.SIZES}
    moved = _check(gpu.SliverChecker(n), n, items, DEFAULT_BUDGET, what=f"n={n} {order}")
    assert moved[3] == 0 and moved[2] == len(items)


@pytest.mark.parametrize("slivers", [1, 2])
@pytest.mark.parametrize("n", [13, 100])
def test_small_budgets(gpu, n, slivers):
    items = R.family_case(n, R.SIZES)
    budget = 1 if slivers == 1 else 2 * M.scratch(n, max(R.SIZES))
    moved = _check(gpu.SliverChecker(n), n, items, budget, what=f"n={n} budget of {slivers}")
    assert moved[0] == len(items) if slivers == 1 else 1 < moved[0] < len(items)
    assert moved[3] == 0


def _blocks(n, items, limit):
    lays = [EP.decode_layout(R.k_of(n, a), n, limit, p) for a, _, p, _ in items]
    return ({len(l.in_blocks) for l in lays}, {len(l.out_blocks) for l in lays},
            sum(EP.pair_precondition(l) for l in lays))


@pytest.mark.parametrize("limit", [16, 8])
def test_lowered_block_limit(gpu, limit):
    """The BATCH_CALLS entries at n = 100 with lowered block limits (the limit is process-wide, so
    a call has one).  Limit 16: both axes, every pattern, jobs of 3 to 8 input and 1 to 5 output
    blocks in one launch; limit 8: the secondary patterns of at most 8 blocks (every primary one
    has more).  With the default limit's calls above (1 to 3 input blocks, jobs that meet the
    pairing precondition and jobs that do not) the launches cover 1 to 8 input blocks."""
    n = 100
    assert {(34, 100, 16, 67, 67), (67, 100, 16, 90, 90), (34, 100, 8, 91, 90)} <= set(EP.BATCH_CALLS)
    items = R.family_case(n, R.SIZES, limit)
    assert len(items) == (67 + 90 if limit == 16 else 90)
    n_in, n_out, _ = _blocks(n, items, limit)
    d_in, _, d_pairs = _blocks(n, R.family_case(n, R.SIZES), None)
    if limit == 16:
        assert n_in == set(range(3, 9)) and n_out == {1, 2, 3, 5}
        assert n_in | d_in == set(range(1, 9)) and 0 < d_pairs < 97
    else:
        assert max(n_in) == 8 and n_out == {1, 2, 3, 4, 5}
    with EP.block_limit(limit):
        moved = _check(gpu.SliverChecker(n), n, items, DEFAULT_BUDGET, limit, f"block limit {limit}")
    assert moved[3] == 0 and moved[2] == len(items)


def test_n1000_two_per_group(gpu):
    n = 1000
    fams = {a: EP.families(R.k_of(n, a), n) for a in R.AXES}
    items = []
    for si, s in enumerate(R.SIZES_1000):
        for ai, a in enumerate(R.AXES):
            for j in range(2):
                q = (7 * (2 * si + j) + 3 * ai) % len(fams[a])
                items.append((a, s, R.handed_over(fams[a][q][1], j), j))
    moved = _check(gpu.SliverChecker(n), n, items, DEFAULT_BUDGET, what="n=1000")
    assert moved == [1, 2 if len({EP.decode_layout(R.k_of(n, a), n, None, p).C
                                  for a, _, p, _ in items}) == 2 else 1, 16, 0, 8]


def test_other_paths(gpu):
    """s = 2 slivers and slivers with every original received take the per-sliver decode, and
    s = 2 the per-size verification, inside the same call; at n = 4500 every sliver takes the
    per-size verification (wide trees) and the primary code's decode has more than 8 blocks."""
    n = 100
    items = R.family_case(n, [2, 6, 130], repeat=1, only_batched=False)[:24]
    for ai, a in enumerate(R.AXES):
        k = R.k_of(n, a)
        items.insert(3 + ai, (a, 66, list(range(k)), 1))              # nothing erased
        items.insert(9 + ai, (a, 2, R.handed_over(range(k), 1), 2))  # nothing erased, shuffled
    pred = R.predicted(n, items, DEFAULT_BUDGET)
    erasing = [sorted(p) != list(range(len(p))) for _, _, p, _ in items]
    assert pred[3] == 4 + sum(e and it[1] == 2 for e, it in zip(erasing, items)) and pred[2] > 0
    moved = _check(gpu.SliverChecker(n), n, items, DEFAULT_BUDGET, what="n=100 other paths")
    assert moved == pred

    n = 4500
    items, paths = [], []
    for ai, a in enumerate(R.AXES):
        k = R.k_of(n, a)
        comb = dict(EP.families(k, n))["comb2"]              # every 2nd shard gone: every block
        paths.append(EP.batch_path(EP.decode_layout(k, n, None, comb), 6))
        items += [(a, 6, R.handed_over(comb, ai), 0), (a, 4, list(range(k)), 1)]
    # the primary code has 9 input blocks there (per-sliver), the secondary one 6 (a range launch)
    assert paths == ["single", "batched"]
    assert R.predicted(n, items, DEFAULT_BUDGET) == [1, 1, 1, 3, 4]
    before = M.stats()
    _check(gpu.SliverChecker(n), n, items, DEFAULT_BUDGET, what="n=4500")
    assert M.moved(before)[1:3] == [0, 4], "trees of 4500 leaves take the per-size verification"


def test_uniform_batch_equals_the_per_size_call(gpu):
    """A batch uniform in size and axis: bytes, roots and verdicts equal what
    rs2_verifier_recover_slivers_device_async writes for it."""
    n, s, axis = 100, 66, "primary"
    k = R.k_of(n, axis)
    items = [(axis, s, R.handed_over(p, j), j % M.POOL)
             for j, (_, p) in enumerate(EP.families(k, n)[:24])]
    m = len(items)
    want = bytearray(R.expected_roots(n, items))
    want[32:64] = want[0:32]                                  # one mismatch among the matches
    s_off, s_size, _, _ = R.layout(n, items)
    sym = np.concatenate([R.received(n, it) for it in items])
    d_sym = torch.tensor(sym, dtype=torch.uint8, device=R.dev())
    outs = []
    for mixed in (False, True):
        d_out = torch.full((m * k * s,), R.FILL, dtype=torch.uint8, device=R.dev())
        d_roots = torch.full((m * 32,), R.FILL, dtype=torch.uint8, device=R.dev())
        d_verdict = torch.full((m,), -1, dtype=torch.int32, device=R.dev())
        pats = [p for _, _, p, _ in items]
        if mixed:
            rc = gpu.SliverChecker(n).recover_async(
                [axis] * m, [s] * m, pats, d_sym.data_ptr(), [i * k * s for i in range(m)],
                d_out.data_ptr(), [i * k * s for i in range(m)], bytes(want), d_roots.data_ptr(),
                d_verdict.data_ptr())
        else:
            rc = gpu.SliverVerifier(n, s, axis).recover_slivers_async(
                pats, d_sym.data_ptr(), d_out.data_ptr(), bytes(want), d_roots.data_ptr(),
                d_verdict.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.last_error())
        outs.append((d_out.cpu().numpy().tobytes(), d_roots.cpu().numpy().tobytes(),
                     d_verdict.cpu().tolist()))
    assert outs[0] == outs[1]
    assert outs[1][2] == [R.MATCH, R.MISMATCH] + [R.MATCH] * (m - 2)
    assert outs[1][0] == b"".join(R.want_sliver(n, it) for it in items)
