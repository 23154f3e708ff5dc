"""The tree cache of rs2_sliver_checker_recovery_symbols_device_async: BUILD into d_nodes, then
CACHED from it, with the counters; a flipped cached node shows in exactly the proofs whose path
holds it while d_nodes stays as passed; the all-zero warming call; an all-systematic CACHED call
expands nothing; the host form; and recovery.recovery_symbols_of_blobs on real blobs of three
lengths against recovery_symbols_for_targets."""
import ctypes

import numpy as np
import pytest
import torch

import symbols_mixed as X
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 100


def _items():
    out = []
    for q, (a, s) in enumerate([("primary", 6), ("secondary", 18), ("primary", 258),
                                ("secondary", 6), ("primary", 6), ("secondary", 4)]):
        k = X.k_of(N, a)
        ts = [[k, 0, N - 1, k - 1], [3, 2, 1], [], [k + 1, 5, 5], [0, k - 1], [N - 1]][q]
        out.append((a, s, q % X.POOL, ts))
    return out


def test_build_then_cached(gpu):
    items = _items()
    L, nn = X.shape(N)
    c = gpu.SliverChecker(N)
    before = X.stats()
    res, sym0, o_off, prf0, nodes0 = X.run(c, N, items, want_nodes=True)
    assert res == 0, _lib.last_error()
    assert X.moved(before) == X.predicted(N, items, "build", True) and X.moved(before)[2] == 6
    X.check_outputs(N, items, sym0, o_off, prf0, nodes0, what="build")
    d_nodes = X.to_dev(nodes0)
    before = X.stats()
    res, sym, _, prf, nodes = X.run(c, N, items, trees="cached", nodes=d_nodes)
    assert res == 0, _lib.last_error()
    delta = X.moved(before)
    # items 1 and 4 ask for systematic symbols only, item 2 for nothing: three are expanded,
    # nothing is built, five slivers are served from the cache
    assert delta == X.predicted(N, items, "cached", True)
    assert delta[1:5] == [3, 0, 5, sum(len(it[3]) for it in items)]
    assert sym.tobytes() == sym0.tobytes() and prf.tobytes() == prf0.tobytes()
    assert nodes.tobytes() == nodes0.tobytes(), "a CACHED call wrote d_nodes"


def test_flipped_node_shows_in_the_proofs_that_hold_it(gpu):
    items = _items()
    L, nn = X.shape(N)
    c = gpu.SliverChecker(N)
    good = np.concatenate([np.frombuffer(w[2], dtype=np.uint8) for w in X.want(N, items)])
    bad = good.copy()
    # sliver 3's leaf 4 is the level-0 sibling of leaf 5 (two of its three requests)
    node = 4
    bad[(3 * nn + node) * 32 + 7] ^= 0x40
    res, sym, o_off, prf, nodes = X.run(c, N, items, trees="cached", nodes=X.to_dev(bad))
    assert res == 0, _lib.last_error()
    assert nodes.tobytes() == bad.tobytes(), "a CACHED call wrote d_nodes"
    want_prf = b"".join(w[1] for w in X.want(N, items))
    got = prf.tobytes()
    j = 0
    for i, it in enumerate(items):
        for t in it[3]:
            same = got[j * L * 32:(j + 1) * L * 32] == want_prf[j * L * 32:(j + 1) * L * 32]
            assert same == (not (i == 3 and t == 5)), (i, t)
            j += 1
    for i, (it, w) in enumerate(zip(items, X.want(N, items))):   # the symbols do not depend on it
        assert sym[o_off[i]:o_off[i] + len(it[3]) * it[1]].tobytes() == w[0], i


def test_warming_call_and_all_systematic_cached(gpu):
    items = _items()
    L, nn = X.shape(N)
    c = gpu.SliverChecker(N)
    warm = [it[:3] + ([],) for it in items]
    before = X.stats()
    res, sym, o_off, prf, nodes = X.run(c, N, warm, want_nodes=True)
    assert res == 0, _lib.last_error()
    assert X.moved(before) == [1, 6, 6, 0, 0, 6]   # gather, 2 encodes, leaves, trees, scatter
    for i, w in enumerate(X.want(N, items)):
        assert nodes[i * nn * 32:(i + 1) * nn * 32].tobytes() == w[2], i
    assert (sym == X.FILL).all() and (prf == X.FILL).all()
    # a BUILD call with no targets and no d_nodes has nothing to do
    before = X.stats()
    res = X.run(c, N, warm)[0]
    assert res == 0 and X.moved(before) == [1, 0, 0, 0, 0, 0]
    # systematic targets only, from the warmed cache: a copy out of the caller's slivers
    systematic = [it[:3] + ([0, X.k_of(N, it[0]) - 1, 1],) for it in items]
    before = X.stats()
    res, sym, o_off, prf, _ = X.run(c, N, systematic, trees="cached", nodes=X.to_dev(nodes))
    assert res == 0, _lib.last_error()
    assert X.moved(before) == [1, 0, 0, 6, 18, 1]  # the request launch alone
    X.check_outputs(N, systematic, sym, o_off, prf, what="systematic")


def test_host_form(gpu):
    items = _items()
    L, _ = X.shape(N)
    m = len(items)
    wants = X.want(N, items)
    keep = [np.ascontiguousarray(X.ref_of(N, it)["data"][it[2]]) for it in items]
    axes = np.array([X.AXES.index(it[0]) for it in items], dtype=np.uint8)
    sizes = (ctypes.c_uint16 * m)(*[it[1] for it in items])
    ptrs = (ctypes.c_void_p * m)(*[a.ctypes.data for a in keep])
    lens = (ctypes.c_uint64 * m)(*[a.size for a in keep])
    counts = (ctypes.c_uint32 * m)(*[len(it[3]) for it in items])
    flat = [t for it in items for t in it[3]]
    ta = (ctypes.c_uint16 * len(flat))(*flat)
    bufs = [np.full(max(len(it[3]) * it[1], 1), X.FILL, np.uint8) for it in items]
    outs = (ctypes.c_void_p * m)(*[b.ctypes.data for b in bufs])
    prf = np.full(len(flat) * L * 32, X.FILL, np.uint8)
    st = (ctypes.c_int * m)()

    def call(status=None):
        return _lib.lib().rs2_recovery_symbols_mixed(N, m, axes.ctypes.data, sizes, ptrs, lens, counts,
                                                     ta, outs, prf.ctypes.data, status)

    assert call() == 0, _lib.last_error()
    for i, (it, w) in enumerate(zip(items, wants)):
        assert bufs[i][:len(it[3]) * it[1]].tobytes() == w[0], i
    assert prf.tobytes() == b"".join(w[1] for w in wants)
    # a wrong length: refused as a whole without status_out, skipped with it
    for b in bufs:
        b[:] = X.FILL
    prf[:] = X.FILL
    lens[3] -= 2
    assert call() == _lib.RS2_E_INCORRECT_DATA_LENGTH
    assert all((b == X.FILL).all() for b in bufs) and (prf == X.FILL).all()
    assert call(st) == 0, _lib.last_error()
    assert list(st) == [0, 0, 0, _lib.RS2_E_INCORRECT_DATA_LENGTH, 0, 0]
    j = 0
    for i, (it, w) in enumerate(zip(items, wants)):
        cnt = len(it[3])
        got = bufs[i][:cnt * it[1]].tobytes(), prf[j * L * 32:(j + cnt) * L * 32].tobytes()
        if i == 3:
            assert got == (bytes([X.FILL]) * (cnt * it[1]), bytes([X.FILL]) * (cnt * L * 32))
        else:
            assert got == (w[0], w[1]), i
        j += cnt


def test_recovery_symbols_of_blobs(gpu):
    """Real blobs of three lengths (three symbol sizes), sources on both axes: what
    recovery_symbols_for_targets returns, from one call."""
    n = 10
    cfg = gpu.ReedSolomonEncodingConfig(n)
    rng = np.random.default_rng(8)
    src, targets, metas = [], [], []
    for length in (300, 1500, 9000):
        blob = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        pairs, meta = cfg.encode_with_metadata(blob)
        for i, ts in ((0, list(range(n))), (4, []), (9, [7, 7, 2])):
            src += [pairs[i].primary, pairs[i].secondary]
            targets += [ts, ts[::-1]]
            metas += [(meta, len(blob))] * 2
    assert len({sl.symbol_size for sl in src}) == 3
    before = X.stats()
    got = gpu.recovery_symbols_of_blobs(cfg, src, targets)
    assert X.moved(before)[0] == 1
    assert got == gpu.recovery_symbols_for_targets(cfg, src, targets)
    for sl, ts, syms, (meta, length) in zip(src, targets, got, metas):
        s = cfg.symbol_size_for_blob(length)
        for tp, sym in zip(ts, syms):
            t_index = tp if sym.axis == gpu.PRIMARY else n - 1 - tp
            sym.verify(n, s, meta.metadata, t_index)
    with pytest.raises(gpu.recovery.RecoverySymbolError):
        gpu.recovery_symbols_of_blobs(cfg, [src[0]], [[n]])
