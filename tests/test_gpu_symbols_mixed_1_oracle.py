"""rs2_sliver_checker_recovery_symbols_device_async against the oracle: every symbol, proof and
tree byte of a mixed call equals symbols_multi.expected / O.merkle_nodes for that sliver's own
(n, size, axis), and equals what rs2_verifier_recovery_symbols_multi_device_async writes when the
same requests are issued per (axis, size).  Shapes: n in {10, 13, 100} (13: the axes' codes differ
in block size), both axes, s in {4, 6, 18, 258}, one to three slivers per group; every target of
every sliver at n = 10; at n = 100 uneven lists with empty slivers, repeats and the K-1 / K seam;
three caller orders; budgets of one and two slivers; the counters against a Python restatement of
the plan; s = 2 and n = 4500 (the per-size path; the C restatement is the reference there);
n = 1000 with two sizes and two slivers each; a uniform batch against the verifier call."""
import ctypes

import numpy as np
import pytest

import symbols_mixed as X
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [4, 6, 18, 258]


def _items(n, lists):
    """One to three slivers per (axis, size) group, the groups interleaved; lists(axis, s, q):
    the targets of the q-th sliver of the group."""
    out = []
    for q in range(3):
        for gi, s in enumerate(SIZES):
            for ai, a in enumerate(X.AXES):
                if q <= (gi + ai) % 3:
                    out.append((a, s, q, lists(a, s, q)))
    return out


def _check(gpu, checker, n, items, trees="build", nodes=None, want_nodes=False, per_size=None,
           what=""):
    res, sym, o_off, prf, got_nodes = X.run(checker, n, items, trees, nodes, want_nodes)
    assert res == 0, _lib.last_error()
    X.check_outputs(n, items, sym, o_off, prf, got_nodes if want_nodes else None, what=what)
    if per_size is not None:
        got = X.got_per_item(n, items, sym, o_off, prf, got_nodes if want_nodes else None)
        for i, (g, w) in enumerate(zip(got, per_size)):
            assert g == w, f"{what}: item {i} {items[i][:3]} differs from the per-size call"
    return sym, o_off, prf, got_nodes


@pytest.mark.parametrize("n", [10, 13])
def test_every_target_of_every_sliver(gpu, n):
    items = _items(n, lambda a, s, q: list(range(n)) if q != 1 else list(range(n - 1, -1, -1)))
    c = gpu.SliverChecker(n)
    per_size = X.run_per_size(gpu, n, items, want_nodes=True)
    before = X.stats()
    _check(gpu, c, n, items, want_nodes=True, per_size=per_size, what=f"n={n}")
    delta = X.moved(before)
    assert delta == X.predicted(n, items, "build", True)
    assert delta[5] <= X.WINDOW_LAUNCHES
    # without trees for the caller: the same symbols and proofs, no scatter
    before = X.stats()
    _check(gpu, c, n, items, what=f"n={n} no nodes")
    assert X.moved(before) == X.predicted(n, items, "build", False)


def _uneven(n):
    def lists(a, s, q):
        k = X.k_of(n, a)
        rng = np.random.default_rng([n, s, q, X.AXES.index(a)])
        if q == 1:
            return []
        if q == 2:
            return [k - 1, k, k, n - 1, 0, k - 1]
        return [k, k - 1] + [int(t) for t in rng.integers(0, n, 9)]
    return lists


@pytest.mark.parametrize("order", ["interleaved", "sorted", "reversed"])
def test_uneven_lists_three_orders(gpu, order):
    n = 100
    items = X.reorder(_items(n, _uneven(n)), order)
    assert any(not it[3] for it in items)
    c = gpu.SliverChecker(n)
    per_size = X.run_per_size(gpu, n, items, want_nodes=True)
    before = X.stats()
    _check(gpu, c, n, items, want_nodes=True, per_size=per_size, what=order)
    assert X.moved(before) == X.predicted(n, items, "build", True)
    before = X.stats()
    _check(gpu, c, n, items, what=order)
    delta = X.moved(before)
    # the empty slivers of a BUILD call without d_nodes do no work
    assert delta == X.predicted(n, items, "build", False)
    assert delta[1] == sum(1 for it in items if it[3])


@pytest.mark.parametrize("hold", [1, 2])
@pytest.mark.parametrize("have_nodes", [False, True])
def test_windows(gpu, hold, have_nodes):
    """Budgets that hold one and two slivers of the largest size: the same bytes as one window."""
    n = 100
    _, nn = X.shape(n)
    items = _items(n, _uneven(n))[:9]
    c = gpu.SliverChecker(n)
    sym0, o_off, prf0, nodes0 = _check(gpu, c, n, items, want_nodes=have_nodes)
    budget = hold * (n * (258 + 32) + nn * 32)
    try:
        gpu.set_verify_mixed_budget(budget)
        before = X.stats()
        sym, _, prf, nodes = _check(gpu, c, n, items, want_nodes=have_nodes, what=f"hold {hold}")
        delta = X.moved(before)
    finally:
        gpu.set_verify_mixed_budget(0)
    want = X.predicted(n, items, "build", have_nodes, budget)
    assert delta == want and want[0] > 1
    assert delta[5] <= want[0] * X.WINDOW_LAUNCHES
    assert sym.tobytes() == sym0.tobytes() and prf.tobytes() == prf0.tobytes()
    if have_nodes:
        assert nodes.tobytes() == nodes0.tobytes()
    before = X.stats()
    _check(gpu, c, n, items)
    assert X.moved(before)[0] == 1      # the default budget is back


def test_two_byte_symbols_take_the_other_path(gpu):
    n = 10
    items = [("primary", 2, 0, list(range(n))), ("secondary", 6, 1, [3, 9, 0]),
             ("secondary", 2, 2, [9, 4, 3, 4]), ("primary", 2, 1, []), ("primary", 18, 0, [7, 6])]
    c = gpu.SliverChecker(n)
    per_size = X.run_per_size(gpu, n, items, want_nodes=True)
    before = X.stats()
    _check(gpu, c, n, items, want_nodes=True, per_size=per_size, what="s=2")
    assert X.moved(before) == X.predicted(n, items, "build", True)
    nodes = X.to_dev(np.concatenate([np.frombuffer(w[2], dtype=np.uint8) for w in X.want(n, items)]))
    _check(gpu, c, n, items, trees="cached", nodes=nodes, what="s=2 cached")


@pytest.fixture(scope="module")
def cpu_port():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_fullsize import load_cpu
    return load_cpu()


def test_wide_trees_take_the_other_path(gpu, cpu_port):
    """n = 4500, one sliver: expanded by the per-size verifier, its tree built a level per launch;
    leaves 4095 / 4096 sit either side of the one-workgroup tree's limit."""
    n, axis = 4500, "secondary"
    k = X.k_of(n, axis)
    items = [(axis, 4, 0, [0, k - 1, k, 4095, 4096, 4499])]
    c = gpu.SliverChecker(n)
    res, sym, o_off, prf, nodes = X.run(c, n, items, want_nodes=True, cpu=cpu_port, pool=1)
    assert res == 0, _lib.last_error()
    X.check_outputs(n, items, sym, o_off, prf, nodes, cpu=cpu_port, pool=1, what="n=4500")


def test_n1000_two_sizes_two_slivers_each(gpu):
    n = 1000
    items = []
    for q in range(2):
        for a, s in (("primary", 20), ("secondary", 66)):
            k = X.k_of(n, a)
            rng = np.random.default_rng([q, s])
            items.append((a, s, q, [0, k - 1, k, n - 1] + [int(t) for t in rng.integers(0, n, 6)]))
    c = gpu.SliverChecker(n)
    per_size = X.run_per_size(gpu, n, items, want_nodes=True, pool=2)
    res, sym, o_off, prf, nodes = X.run(c, n, items, want_nodes=True, pool=2)
    assert res == 0, _lib.last_error()
    X.check_outputs(n, items, sym, o_off, prf, nodes, pool=2, what="n=1000")
    assert X.got_per_item(n, items, sym, o_off, prf, nodes) == per_size


def test_uniform_batch_equals_the_verifier_call(gpu):
    n, s, a = 100, 18, "primary"
    k = X.k_of(n, a)
    items = [(a, s, q, ts) for q, ts in enumerate([[k, 0, 99], [], [5, 5, k - 1, 98, 1]])]
    c = gpu.SliverChecker(n)
    per_size = X.run_per_size(gpu, n, items, want_nodes=True)
    before = X.stats()
    _check(gpu, c, n, items, want_nodes=True, per_size=per_size, what="uniform")
    assert X.moved(before) == [1, 3, 3, 0, 8, 6]


def test_requests_of_more_than_one_chunk(gpu):
    """A window of 2^20 + 13 requests: the second chunk's table takes the first one's place, its
    entries are requests 2^20 .. of the call, and a sliver's symbols cross the chunk edge.  One
    small sliver repeats its targets (s = 2, n = 10), a sliver before it and one after it."""
    n = 10
    L, nn = X.shape(n)
    reps = (X.REQUEST_CHUNK + 4) // n
    big = [t for _ in range(reps) for t in range(n)][:X.REQUEST_CHUNK + 4]
    items = [("secondary", 6, 1, [9, 0, 4, 4]), ("primary", 2, 0, big), ("primary", 18, 2, [7, 8, 0, 1, 6])]
    total = sum(len(it[3]) for it in items)
    assert total == X.REQUEST_CHUNK + 13
    c = gpu.SliverChecker(n)
    before = X.stats()
    res, sym, o_off, prf, _ = X.run(c, n, items)
    assert res == 0, _lib.last_error()
    # gather, two encodes (s = 2 takes the per-size path), leaves, trees, two request chunks
    assert X.moved(before) == X.predicted(n, items) == [1, 3, 3, 0, total, 7]
    # the oracle's bytes, assembled with numpy: ten distinct (symbol, proof) pairs, repeated
    one = X.want(n, [items[1][:3] + (list(range(n)),)])[0]
    per_sym = np.frombuffer(one[0], dtype=np.uint8).reshape(n, 2)
    per_prf = np.frombuffer(one[1], dtype=np.uint8).reshape(n, L * 32)
    idx = np.array(big)
    small = X.want(n, [items[0], items[2]])
    assert sym[o_off[0]:o_off[0] + 24].tobytes() == small[0][0]
    assert sym[o_off[1]:o_off[1] + 2 * len(big)].tobytes() == per_sym[idx].tobytes()
    assert sym[o_off[2]:o_off[2] + 90].tobytes() == small[1][0]
    assert prf[:4 * L * 32].tobytes() == small[0][1]
    assert prf[4 * L * 32:(4 + len(big)) * L * 32].tobytes() == per_prf[idx].tobytes()
    assert prf[(4 + len(big)) * L * 32:].tobytes() == small[1][1]
    keep = np.ones(sym.size, dtype=bool)
    for o, it in zip(o_off, items):
        keep[o:o + len(it[3]) * it[1]] = False
    assert (sym[keep] == X.FILL).all()
