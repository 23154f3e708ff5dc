"""Mixed sliver verification against the oracle (rs2_sliver_checker_verify_device_async): one call
over slivers that share only n_shards -- every symbol size of the list on both axes -- must give,
per sliver and in the caller's order, the oracle's Merkle root of those bytes.

Geometries: n = 10 (C = 4; primary high rate with 2 input blocks and 1 output block, secondary the
shared-input path), n = 13 (both axes high rate, 3 input blocks), n = 100 (C = 64), n = 1000
(C = 512, 1000-leaf trees; sizes {2, 20, 66, 130, 1206}).  The sizes cross the codec's 64-byte
chunk rule (tail only, exactly one chunk, chunk + 2-byte tail), the leaf message's one, two and
three Blake2b blocks and s = 6, where several lines share one 64-pair tile.  Counts: 1 and 5 slivers
per group, and 65 in one group beside singletons (trees run four per workgroup); caller orders
interleaved, sorted and reverse.  The same input under budgets that hold 1 and 2 slivers of the
largest size splits groups across windows and must give the same roots.

rs2_verify_mixed_stats pins the path: inputs with every s >= 4 never take the per-size path; the
launch counter moves by at most RS2_VERIFY_MIXED_WINDOW_LAUNCHES for the 22 groups of one n = 100
window, and by the same amount for 1 and for 5 slivers per group.  s = 2 and n = 4500 (trees wider
than 4096 leaves) are ineligible by the planner's rule (tests/test_planner_groups.py) and take the
per-size path inside the same call."""
import numpy as np
import pytest
import torch

import verify_mixed as M

pytestmark = pytest.mark.gpu

GEOMETRIES = [10, 13, 100, 1000]


@pytest.fixture(scope="module")
def checkers(gpu):
    made = {}

    def get(n):
        if n not in made:
            made[n] = gpu.SliverChecker(n)
        return made[n]
    yield get
    made.clear()


def _check(checker, n, items, what):
    rc, roots, _ = M.run(checker, n, items)
    assert rc == 0, (rc, M._lib.last_error())
    M.check_roots(n, items, roots, what=what)
    return roots


@pytest.mark.parametrize("order", ["interleaved", "sorted", "reverse"])
@pytest.mark.parametrize("per", [1, 5])
@pytest.mark.parametrize("n", GEOMETRIES)
def test_every_size_both_axes(checkers, n, per, order):
    sizes = M.sizes_of(n)
    items = M.groups_case(n, sizes, per, order)
    before = M.stats()
    _check(checkers(n), n, items, f"n={n} per={per} {order}")
    windows, grouped, single, groups, launches = M.moved(before)
    # s = 2 is the one ineligible size: its two groups take the per-size path, nothing else does
    assert windows == 1 and groups == 2 * len(sizes)
    assert single == 2 * per and grouped == len(items) - 2 * per
    assert launches <= M.LAUNCHES


@pytest.mark.parametrize("n", GEOMETRIES)
def test_big_group_beside_singletons(checkers, n):
    sizes = [s for s in M.sizes_of(n) if s >= 4]
    big = ("primary", sizes[1], 65)
    items = M.groups_case(n, sizes, 1, "interleaved", big=big)
    assert len(items) == 2 * len(sizes) + 64
    before = M.stats()
    _check(checkers(n), n, items, f"n={n} 65 in one group")
    assert M.moved(before)[2] == 0                      # every s >= 4: no per-size path


@pytest.mark.parametrize("n", GEOMETRIES)
def test_windows_split_groups(checkers, n):
    sizes = M.sizes_of(n)
    items = M.groups_case(n, sizes, 5, "interleaved")
    whole = _check(checkers(n), n, items, f"n={n} one window")
    try:
        for hold in (1, 2):
            M.set_budget(hold * M.scratch(n, max(sizes)))
            before = M.stats()
            got = _check(checkers(n), n, items, f"n={n} budget of {hold}")
            assert got == whole
            windows, _, _, groups, launches = M.moved(before)
            assert windows >= 2 and groups > 2 * len(sizes)   # groups were split across windows
            assert launches <= M.LAUNCHES * windows
    finally:
        M.set_budget(0)


def test_stats_eligible_sizes_n100(checkers):
    """The 11 sizes >= 4 on both axes at n = 100, one window: no per-size path, at most the
    header's launches, and as many launches for 5 slivers per group as for 1."""
    n = 100
    sizes = [s for s in M.SIZES if s >= 4]
    assert len(sizes) == 11
    moves = []
    for per in (1, 5):
        items = M.groups_case(n, sizes, per, "interleaved")
        before = M.stats()
        _check(checkers(n), n, items, f"n=100 eligible per={per}")
        moves.append(M.moved(before))
    for per, (windows, grouped, single, groups, launches) in zip((1, 5), moves):
        assert windows == 1 and groups == 22 and single == 0 and grouped == 22 * per
        assert 1 <= launches <= M.LAUNCHES
    assert moves[0][4] == moves[1][4]


def test_n1000_against_the_per_size_verifier(gpu, checkers):
    """One root per (size, axis) at n = 1000 also equals rs2_verifier_roots_device_async's."""
    n = 1000
    items = M.groups_case(n, M.SIZES_1000, 1, "sorted")
    roots = _check(checkers(n), n, items, "n=1000")
    for i, (axis, s, seed) in enumerate(items):
        v = gpu.SliverVerifier(n, s, axis)
        d_in = torch.tensor(M.sliver(n, s, axis, seed), dtype=torch.uint8, device=M.dev())
        d_out = torch.zeros(32, dtype=torch.uint8, device=M.dev())
        v.roots_async(1, d_in.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == roots[32 * i:32 * i + 32], (axis, s)


def test_two_byte_symbols_take_the_declared_path(checkers):
    """s = 2 is ineligible by the planner's rule: the per-size path, the oracle's roots."""
    for n in (10, 100):
        items = [(a, 2, j) for j in range(3) for a in M.AXES]
        before = M.stats()
        _check(checkers(n), n, items, f"n={n} s=2")
        windows, grouped, single, groups, _ = M.moved(before)
        assert (windows, grouped, single, groups) == (1, 0, 6, 2)


def test_wide_trees_fall_back(checkers):
    """n = 4500: trees of more than 4096 leaves are ineligible; the roots are the C restatement's
    and all four slivers take the per-size path."""
    n = 4500
    items = [(a, s, 0) for s in (4, 66) for a in M.AXES]
    before = M.stats()
    _check(checkers(n), n, items, "n=4500")
    windows, grouped, single, groups, _ = M.moved(before)
    assert (windows, grouped, single, groups) == (1, 0, 4, 4)


def test_host_form_and_python_mirror(gpu):
    n = 13
    cfg = gpu.ReedSolomonEncodingConfig(n)
    items = M.groups_case(n, [2, 6, 66, 130], 2, "reverse")
    slivers = [gpu.SliverData(gpu.Symbols(M.sliver(n, s, a, seed).tobytes(), s), 0, a)
               for a, s, seed in items]
    roots = gpu.sliver_merkle_roots_mixed(cfg, slivers)
    assert b"".join(roots) == M.expected_roots(n, items)
    assert gpu.sliver_merkle_roots_mixed(cfg, []) == []
    with pytest.raises(ValueError):                      # the uniform call keeps its rule
        gpu.sliver_merkle_roots(cfg, slivers[:4])
    assert np.all(np.array(list(gpu.verify_mixed_stats().values())) >= 0)
