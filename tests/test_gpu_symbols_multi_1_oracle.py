"""rs2_verifier_recovery_symbols_multi_device_async against the oracle: every symbol and proof
byte equals O.recovery_symbols / O.merkle_proof (the C restatement's rs2cpu_recovery_symbol at
n = 4500), the trees equal O.merkle_nodes, and the same requests through the existing per-request
call (the source sliver passed once per target) give the same bytes.  Shapes: every target of
every sliver at n in {4, 7, 10} (padded odd levels, the last odd leaf, the k-1 / k seam); uneven
count lists with empty slivers, duplicates and unsorted targets at n = 100; a symbol longer than
one pass of a wave (s = 1206) at n = 1000; the per-level tree path at n = 4500; windows of one and
two slivers; the host form and the Python API."""
import ctypes

import numpy as np
import pytest

import rs2_oracle as O
import symbols_multi as M
from walrus_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu_port():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_fullsize import load_cpu
    lib = load_cpu()
    P = ctypes.c_void_p
    lib.rs2cpu_recovery_symbol.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, P,
                                           ctypes.c_uint32, P, P]
    return lib


@pytest.mark.parametrize("axis", M.AXES)
@pytest.mark.parametrize("s", [2, 6])
@pytest.mark.parametrize("n", [4, 7, 10])
def test_every_target_of_every_sliver(gpu, n, s, axis):
    ref = M.reference(n, s, axis, 3)
    v = gpu.SliverVerifier(n, s, axis)
    M.check(v, ref, [list(range(n))] * 3, want_nodes=True)
    M.check(v, ref, [list(range(n - 1, -1, -1)), [], [n - 1, 0]])


@pytest.mark.parametrize("axis", M.AXES)
def test_uneven_lists_with_duplicates(gpu, axis):
    n, s = 100, 20
    k = M.k_of(n, axis)
    ref = M.reference(n, s, axis, 6)
    rng = np.random.default_rng(5)
    targets = [[], [k], [int(t) for t in rng.integers(0, n, 100)], [n - 1, k - 1, k], [],
               [int(t) for t in rng.permutation(n)[:17]]]
    targets[2][:6] = [k, k - 1, n - 1, 0, k, k]   # the seam, the last leaf, duplicates
    assert [len(t) for t in targets] == [0, 1, 100, 3, 0, 17]
    v = gpu.SliverVerifier(n, s, axis)
    before = M.stats()
    M.check(v, ref, targets, single=False)
    # windows, slivers expanded, trees built, trees from a cache, requests: the empty slivers of
    # a BUILD call without d_nodes do no work
    assert M.moved(before) == [1, 4, 4, 0, 121]
    M.check(v, ref, targets, want_nodes=True)


def test_symbol_longer_than_a_wave_pass(gpu):
    n, s, axis = 1000, 1206, "primary"
    k = M.k_of(n, axis)
    ref = M.reference(n, s, axis, 4)
    rng = np.random.default_rng(6)
    targets = [[0, k - 1, k, n - 1] + [int(t) for t in rng.integers(0, n, 8)] for _ in range(4)]
    v = gpu.SliverVerifier(n, s, axis)
    M.check(v, ref, targets, want_nodes=True)


@pytest.mark.parametrize("axis", M.AXES)
def test_wide_trees(gpu, cpu_port, axis):
    """n = 4500: node arrays built a level per launch; leaves 4095 / 4096 sit either side of the
    one-workgroup tree's limit.  Symbols and proofs from rs2cpu_recovery_symbol."""
    n, s = 4500, 2
    k = M.k_of(n, axis)
    L, _ = M.shape(n)
    ref = M.reference(n, s, axis, 2, cpu=cpu_port)
    targets = [[0, k - 1, k, 4095, 4096, 4499]] * 2
    v = gpu.SliverVerifier(n, s, axis)
    rc, sym, prf, nodes = M.check(v, ref, targets, want_nodes=True)
    one_sym, one_prf = np.zeros(s, np.uint8), np.zeros(L * 32, np.uint8)
    j = 0
    for i, ts in enumerate(targets):
        for t in ts:
            assert cpu_port.rs2cpu_recovery_symbol(n, s, M.AXES.index(axis),
                                                   ref["data"][i].ctypes.data, t,
                                                   one_sym.ctypes.data, one_prf.ctypes.data) == L
            assert sym[j * s:(j + 1) * s].tobytes() == one_sym.tobytes(), (i, t)
            assert prf[j * L * 32:(j + 1) * L * 32].tobytes() == one_prf.tobytes(), (i, t)
            j += 1


@pytest.mark.parametrize("hold", [1, 2])
@pytest.mark.parametrize("have_nodes", [False, True])
def test_windows(gpu, hold, have_nodes):
    """Budgets that hold one and two slivers: the same bytes as one window, stats slot 0 moves by
    ceil(5 / hold).  Scratch per sliver: (n - k) * s repair bytes, n * 32 leaves, and the node
    array when the caller takes none."""
    n, s, axis = 100, 6, "primary"
    k = M.k_of(n, axis)
    _, nn = M.shape(n)
    ref = M.reference(n, s, axis, 5)
    targets = [[k, 0, 99], [], [5, 5, k - 1, 98, 1], [k + 1], [3, 2, 1, 0]]
    v = gpu.SliverVerifier(n, s, axis)
    _, sym0, prf0, nodes0 = M.check(v, ref, targets, want_nodes=have_nodes, single=False)
    per = (n - k) * s + n * 32 + (0 if have_nodes else nn * 32)
    try:
        gpu.set_recovery_symbols_budget(per * (hold + 1) - 1)
        before = M.stats()
        _, sym, prf, nodes = M.check(v, ref, targets, want_nodes=have_nodes, single=False)
        delta = M.moved(before)
    finally:
        gpu.set_recovery_symbols_budget(0)
    assert delta[0] == -(-5 // hold) and delta[4] == 13
    assert delta[1] == delta[2] == (5 if have_nodes else 4)
    assert sym.tobytes() == sym0.tobytes() and prf.tobytes() == prf0.tobytes()
    if have_nodes:
        assert nodes.tobytes() == nodes0.tobytes()
    before = M.stats()
    M.check(v, ref, targets, single=False)
    assert M.moved(before)[0] == 1      # the default budget is back


def test_host_form_and_length_error(gpu):
    n, s, axis = 10, 6, "secondary"
    ref = M.reference(n, s, axis, 3)
    L, _ = M.shape(n)
    targets = [[9, 0, 4], [], [3, 4, 4, 9]]
    counts = (ctypes.c_uint32 * 3)(*[len(t) for t in targets])
    flat = [t for ts in targets for t in ts]
    ta = (ctypes.c_uint16 * len(flat))(*flat)
    keep = [np.ascontiguousarray(ref["data"][i]) for i in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in keep])
    lens = (ctypes.c_uint64 * 3)(*[a.size for a in keep])
    sym = np.full(len(flat) * s, M.FILL, np.uint8)
    prf = np.full(len(flat) * L * 32, M.FILL, np.uint8)
    rc = _lib.lib().rs2_recovery_symbols_multi(n, s, 1, 3, ptrs, lens, counts, ta, sym.ctypes.data,
                                               prf.ctypes.data)
    assert rc == 0, _lib.last_error()
    want_sym, want_prf = M.expected(ref, targets)
    assert sym.tobytes() == want_sym.tobytes() and prf.tobytes() == want_prf.tobytes()
    # a wrong length and a null sliver: refused, outputs untouched
    sym[:], prf[:] = M.FILL, M.FILL
    lens[1] -= 2
    assert _lib.lib().rs2_recovery_symbols_multi(
        n, s, 1, 3, ptrs, lens, counts, ta, sym.ctypes.data,
        prf.ctypes.data) == _lib.RS2_E_INCORRECT_DATA_LENGTH
    lens[1] += 2
    ptrs[2] = None
    assert _lib.lib().rs2_recovery_symbols_multi(
        n, s, 1, 3, ptrs, lens, counts, ta, sym.ctypes.data,
        prf.ctypes.data) == _lib.RS2_E_INCORRECT_DATA_LENGTH
    ptrs[2] = keep[2].ctypes.data
    ta[0] = n
    assert _lib.lib().rs2_recovery_symbols_multi(
        n, s, 1, 3, ptrs, lens, counts, ta, sym.ctypes.data, prf.ctypes.data) == M.INVALID
    assert (sym == M.FILL).all() and (prf == M.FILL).all()


def test_python_api_round_trip(gpu):
    """recovery.recovery_symbols_for_targets on the slivers of a real encode at n = 10: every
    RecoverySymbol verifies against the blob's metadata for its target and equals what
    recovery_symbols_for_requests returns for the same (source, target) pair."""
    n = 10
    cfg = gpu.ReedSolomonEncodingConfig(n)
    blob = np.random.default_rng(8).integers(0, 256, 1500, dtype=np.uint8).tobytes()
    pairs, meta = cfg.encode_with_metadata(blob)
    s = cfg.symbol_size_for_blob(len(blob))
    for pick, other in ((lambda p: p.primary, gpu.SECONDARY), (lambda p: p.secondary, gpu.PRIMARY)):
        src = [pick(pairs[i]) for i in (0, 4, 9)]
        targets = [list(range(n)), [], [7, 7, 2]]
        got = gpu.recovery_symbols_for_targets(cfg, src, targets)
        assert [len(g) for g in got] == [n, 0, 3]
        for sl, ts, syms in zip(src, targets, got):
            singles = gpu.recovery_symbols_for_requests(cfg, [sl] * len(ts), ts)
            for tp, sym, one in zip(ts, syms, singles):
                assert sym == one
                assert sym.axis == other and sym.index == sl.index
                # the target sliver's index on its own axis (lib.rs:485-503)
                t_index = tp if other == gpu.PRIMARY else n - 1 - tp
                sym.verify(n, s, meta.metadata, t_index)
                with pytest.raises(gpu.recovery.SymbolVerificationError):
                    sym.verify(n, s, meta.metadata, (t_index + 1) % n)
    with pytest.raises(gpu.recovery.RecoverySymbolError):
        gpu.recovery_symbols_for_targets(cfg, [pairs[0].primary], [[n]])
