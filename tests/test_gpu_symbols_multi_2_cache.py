"""The cached trees of rs2_verifier_recovery_symbols_multi_device_async: a BUILD call hands the
node arrays out, a CACHED call serves the same requests from them without hashing (the stats
counters say so), a call whose targets are all systematic launches no codec, and a flipped byte in
one cached node shows in exactly the proofs whose path holds that node -- the cache is read, not
rebuilt, and never written.  A BUILD call with no targets warms the cache."""
import numpy as np
import pytest

import symbols_multi as M

pytestmark = pytest.mark.gpu

N, S = 100, 20


def _targets(k, n):
    rng = np.random.default_rng(21)
    return [[0, k - 1, k, n - 1] + [int(t) for t in rng.integers(0, n, 6)] for _ in range(4)]


@pytest.mark.parametrize("axis", M.AXES)
def test_build_then_cached(gpu, axis):
    k = M.k_of(N, axis)
    ref = M.reference(N, S, axis, 4)
    targets = _targets(k, N)
    total = sum(len(t) for t in targets)
    v = gpu.SliverVerifier(N, S, axis)
    before = M.stats()
    _, sym, prf, nodes = M.check(v, ref, targets, want_nodes=True, single=False)
    assert M.moved(before) == [1, 4, 4, 0, total]
    cache = M.to_dev(nodes)
    before = M.stats()
    _, sym2, prf2, nodes2 = M.check(v, ref, targets, trees="cached", nodes=cache, single=False)
    # repair targets: the codec ran for the four slivers; no tree built, four taken from the cache
    assert M.moved(before) == [1, 4, 0, 4, total]
    assert sym2.tobytes() == sym.tobytes() and prf2.tobytes() == prf.tobytes()
    assert nodes2.tobytes() == nodes.tobytes()


@pytest.mark.parametrize("axis", M.AXES)
def test_cached_systematic_targets_launch_no_codec(gpu, axis):
    k = M.k_of(N, axis)
    ref = M.reference(N, S, axis, 4)
    targets = [[0, k - 1, 5, 5], [k - 1], [], [int(t) for t in range(k - 1, -1, -7)]]
    v = gpu.SliverVerifier(N, S, axis)
    cache = M.to_dev(ref["nodes"][:4])
    before = M.stats()
    M.check(v, ref, targets, trees="cached", nodes=cache, single=False)
    delta = M.moved(before)
    assert delta[1] == 0 and delta[2] == 0 and delta[3] == 3
    # one repair target in one sliver: that sliver alone is expanded
    targets[1] = [k - 1, k]
    before = M.stats()
    M.check(v, ref, targets, trees="cached", nodes=cache, single=False)
    assert M.moved(before)[1:4] == [1, 0, 3]


def test_flipped_cached_node_shows_in_its_proofs_only(gpu):
    axis = "primary"
    k = M.k_of(N, axis)
    L, nn = M.shape(N)
    ref = M.reference(N, S, axis, 4)
    # sliver 2, level 1: the sibling of leaf 10's parent (node 5 of level 1) is node 4, which is
    # on the paths of leaves 10 and 11 and of no other leaf
    level, sib = 1, 4
    at = 2 * nn * 32 + (N + sib) * 32 + 13     # level 1 starts at node N (N is even)
    targets = [[10, 11, 8], [10], [10, 11, 8, 9, 12, k, 10], [11]]
    v = gpu.SliverVerifier(N, S, axis)
    cached = np.array(ref["nodes"][:4]).reshape(-1)
    cached[at] ^= 0x40
    cache = M.to_dev(cached)
    rc, sym, prf, nodes = M.run(v, ref, targets, trees="cached", nodes=cache)
    assert rc == 0
    want_sym, want_prf = M.expected(ref, targets)
    assert sym.tobytes() == want_sym.tobytes()
    assert nodes.tobytes() == cached.tobytes(), "a CACHED call wrote d_nodes"
    differs = np.nonzero(prf != want_prf)[0]
    flat = [(i, t) for i, ts in enumerate(targets) for t in ts]
    hit = [j for j, (i, t) in enumerate(flat) if i == 2 and t in (10, 11)]
    assert len(hit) == 3
    assert differs.tolist() == [(j * L + level) * 32 + 13 for j in hit]
    assert all(prf[d] == want_prf[d] ^ 0x40 for d in differs)


@pytest.mark.parametrize("axis", M.AXES)
def test_warming_call_builds_every_tree(gpu, axis):
    ref = M.reference(N, S, axis, 4)
    v = gpu.SliverVerifier(N, S, axis)
    before = M.stats()
    rc, sym, prf, nodes = M.run(v, ref, [[], [], [], []], want_nodes=True)
    assert rc == 0 and sym.size == 0 and prf.size == 0
    assert nodes.tobytes() == ref["nodes"][:4].tobytes()
    assert M.moved(before) == [1, 4, 4, 0, 0]
    # without d_nodes the same call has nothing to do
    before = M.stats()
    assert M.run(v, ref, [[], [], [], []])[0] == 0
    assert M.moved(before)[1:] == [0, 0, 0, 0]
