"""rs2_sliver_checker_recovery_symbols_device_async inside guard bands (tests/guarded.py): the
sliver, symbol, proof and tree buffers are interiors of larger patterned allocations, the slivers'
symbol extents lie 6 bytes apart, and slivers and symbols sit at placements whose difference mod 16
sends the symbol copy down each of its widths (0: 16-byte pieces where a symbol's two ends agree,
4: 4-byte pieces, 2 / 6: 2-byte pieces; s = 2, 6 and 18 ride in the same call, so edges of every
length occur).  Nothing outside the stated extents may change, CACHED leaves d_nodes as it was, and
a second run with another guard fill gives the same bytes: no result depends on a byte outside an
input's extent.  Then every per-sliver refusal leaves its slots at the fill, and every whole-call
refusal returns its code with the outputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import symbols_mixed as X
from guarded import Guarded
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 10


def _items():
    out = []
    for q, (a, s) in enumerate([("primary", 2), ("secondary", 18), ("primary", 6), ("secondary", 2),
                                ("primary", 18), ("secondary", 6), ("primary", 6)]):
        k = X.k_of(N, a)
        ts = [list(range(N)), [N - 1, k, k - 1, 0, k], [], list(range(N - 1, -1, -1)), [0, 1, 2],
              [k, k], list(range(N))][q]
        out.append((a, s, q % X.POOL, ts))
    return out


def _run(c, items, d_in, d_out, fill, trees, cached_nodes=None):
    dev = X.dev()
    L, nn = X.shape(N)
    m = len(items)
    total = sum(len(it[3]) for it in items)
    i_off, i_size, o_off, o_size = X.layout(N, items)
    data = X.payload(N, items, i_off, i_size, fill=fill)
    slivers = Guarded(i_size, d_in, dev, fill).set(data)
    sym = Guarded(o_size, d_out, dev, 77)
    prf = Guarded(total * L * 32, 0, dev, 78)
    nodes = Guarded(m * nn * 32, 0, dev, fill + 2)
    if cached_nodes is not None:
        nodes.set(np.array(cached_nodes))
    torch.cuda.synchronize()
    rc = X.call_raw(c, items, slivers.ptr, i_off, sym.ptr, o_off, prf.ptr, nodes.ptr, trees)
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    slivers.assert_guards_intact(what="d_slivers")
    assert slivers.numpy().tobytes() == data.tobytes(), "d_slivers was written"
    sym.assert_guards_intact([(o, len(it[3]) * it[1]) for o, it in zip(o_off, items)],
                             what="d_symbols")
    prf.assert_guards_intact(what="d_proofs")
    nodes.assert_guards_intact(what="d_nodes")
    return sym.numpy(), o_off, prf.numpy(), nodes.numpy()


@pytest.mark.parametrize("d_out", [0, 4, 6])
@pytest.mark.parametrize("d_in", [0, 2])
def test_inside_guards(gpu, d_in, d_out):
    items = _items()
    wants = X.want(N, items)
    want_nodes = b"".join(w[2] for w in wants)
    want_prf = b"".join(w[1] for w in wants)
    c = gpu.SliverChecker(N)
    for fill in (11, 151):
        for trees, cached in (("build", None), ("cached", np.frombuffer(want_nodes, dtype=np.uint8))):
            sym, o_off, prf, nodes = _run(c, items, d_in, d_out, fill, trees, cached)
            for i, (it, w) in enumerate(zip(items, wants)):
                got = sym[o_off[i]:o_off[i] + len(it[3]) * it[1]].tobytes()
                assert got == w[0], (trees, fill, i)
            assert prf.tobytes() == want_prf, (trees, fill)
            assert nodes.tobytes() == want_nodes, (trees, fill)


def test_per_sliver_refusals_leave_their_slots(gpu):
    items = _items()
    L, nn = X.shape(N)
    c = gpu.SliverChecker(N)
    bad = list(items)
    bad[0] = (2,) + items[0][1:]                       # an axis that is not one of the two
    bad[1] = (items[1][0], 0) + items[1][2:]           # symbol size 0
    bad[4] = (items[4][0], 7) + items[4][2:]           # an odd symbol size
    bad[5] = items[5][:3] + ([3, N],)                  # a target = n_shards
    skipped = {0, 1, 4, 5}
    codes = {0: X.INVALID, 1: _lib.RS2_E_INCOMPATIBLE_PARAMETERS,
             4: _lib.RS2_E_INCOMPATIBLE_PARAMETERS, 5: X.INVALID}
    # the layout and payload of the valid items: the refused ones' bytes are never looked at
    i_off, i_size, o_off, o_size = X.layout(N, items)
    total = sum(len(it[3]) for it in bad)
    d_sl = X.to_dev(X.payload(N, items, i_off, i_size))
    for trees in ("build", "cached"):
        d_sym = torch.full((o_size,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_prf = torch.full((total * L * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_nodes = torch.full((len(items) * nn * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        if trees == "cached":
            for i, w in enumerate(X.want(N, items)):
                if i not in skipped:
                    d_nodes[i * nn * 32:(i + 1) * nn * 32] = X.to_dev(np.frombuffer(w[2], np.uint8))
        torch.cuda.synchronize()
        # without status_out: the first failing code, nothing runs
        assert X.call_raw(c, bad, d_sl.data_ptr(), i_off, d_sym.data_ptr(), o_off, d_prf.data_ptr(),
                          d_nodes.data_ptr(), trees) == X.INVALID
        torch.cuda.synchronize()
        assert bool((d_sym == X.FILL).all()) and bool((d_prf == X.FILL).all())
        before = X.stats()
        st = X.call_raw(c, bad, d_sl.data_ptr(), i_off, d_sym.data_ptr(), o_off, d_prf.data_ptr(),
                        d_nodes.data_ptr(), trees, statuses=True)
        torch.cuda.synchronize()
        assert st == [codes.get(i, 0) for i in range(len(bad))]
        accepted = [i not in skipped for i in range(len(bad))]
        assert X.moved(before)[:5] == X.predicted(N, bad, trees, True, accepted=accepted)[:5]
        # the refused items' extents are those of the list handed over
        _, _, o_bad, _ = X.layout(N, items)
        X.check_outputs(N, [b if i in skipped else it for i, (it, b) in enumerate(zip(items, bad))],
                        d_sym.cpu().numpy(), o_bad, d_prf.cpu().numpy(), d_nodes.cpu().numpy(),
                        skipped=skipped, what=trees)
    # odd offsets: on freshly filled buffers, the refused sliver's extent and proof slots stay
    for which, at in (("in", 1), ("out", 4)):
        io, oo = list(i_off), list(o_off)
        (io if which == "in" else oo)[at] += 1
        d_sym = torch.full((o_size,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_prf = torch.full((total * L * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_nodes = torch.full((len(items) * nn * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        torch.cuda.synchronize()
        assert X.call_raw(c, items, d_sl.data_ptr(), io, d_sym.data_ptr(), oo, d_prf.data_ptr(),
                          d_nodes.data_ptr(), "build") == X.INVALID
        st = X.call_raw(c, items, d_sl.data_ptr(), io, d_sym.data_ptr(), oo, d_prf.data_ptr(),
                        d_nodes.data_ptr(), "build", statuses=True)
        torch.cuda.synchronize()
        assert st == [X.INVALID if i == at else 0 for i in range(len(items))], which
        X.check_outputs(N, items, d_sym.cpu().numpy(), o_off, d_prf.cpu().numpy(),
                        d_nodes.cpu().numpy(), skipped={at}, what="odd " + which)


def test_every_sliver_refused(gpu):
    """Refused slivers with targets and no accepted one -- the smallest case is one sliver whose
    target, remote input, is n_shards: RS2_OK with status_out, nothing enqueued, the outputs at
    the fill and the counters where they were; device form and host form, both modes."""
    L, nn = X.shape(N)
    c = gpu.SliverChecker(N)
    cases = [[("primary", 6, 0, [3, N])],
             [("primary", 6, 0, [3, N]), (2, 18, 1, [1]), ("secondary", 5, 2, [0, 1, 2])]]
    for items in cases:
        valid = [("primary", 6, 0, it[3]) for it in items]
        i_off, i_size, o_off, o_size = X.layout(N, valid)
        total = sum(len(it[3]) for it in items)
        d_sl = X.to_dev(X.payload(N, [v[:3] + ([],) for v in valid], i_off, i_size))
        d_sym = torch.full((o_size,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_prf = torch.full((total * L * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        d_nodes = torch.full((len(items) * nn * 32,), X.FILL, dtype=torch.uint8, device=X.dev())
        torch.cuda.synchronize()
        for trees in ("build", "cached"):
            before = X.stats()
            st = X.call_raw(c, items, d_sl.data_ptr(), i_off, d_sym.data_ptr(), o_off,
                            d_prf.data_ptr(), d_nodes.data_ptr(), trees, statuses=True)
            torch.cuda.synchronize()
            assert all(code != 0 for code in st) and st[0] == X.INVALID, (trees, st)
            assert X.moved(before) == [0] * 6, trees
            for name, buf in (("d_symbols", d_sym), ("d_proofs", d_prf), ("d_nodes", d_nodes)):
                assert bool((buf == X.FILL).all()), (trees, name)
    # host form
    items = cases[0]
    keep = np.ascontiguousarray(X.ref_of(N, items[0])["data"][0])
    axes = np.array([0], dtype=np.uint8)
    ptrs = (ctypes.c_void_p * 1)(keep.ctypes.data)
    sym = np.full(2 * 6, X.FILL, np.uint8)
    outs = (ctypes.c_void_p * 1)(sym.ctypes.data)
    prf = np.full(2 * L * 32, X.FILL, np.uint8)
    st = (ctypes.c_int * 1)()
    before = X.stats()
    rc = _lib.lib().rs2_recovery_symbols_mixed(
        N, 1, axes.ctypes.data, (ctypes.c_uint16 * 1)(6), ptrs, (ctypes.c_uint64 * 1)(keep.size),
        (ctypes.c_uint32 * 1)(2), (ctypes.c_uint16 * 2)(3, N), outs, prf.ctypes.data, st)
    assert rc == 0 and st[0] == X.INVALID, (rc, st[0], _lib.last_error())
    assert X.moved(before) == [0] * 6
    assert (sym == X.FILL).all() and (prf == X.FILL).all()


def test_whole_call_refusals_leave_outputs_untouched(gpu):
    items = _items()[:3]
    L, nn = X.shape(N)
    dev = X.dev()
    i_off, i_size, o_off, o_size = X.layout(N, items)
    total = sum(len(it[3]) for it in items)
    d_sl = X.to_dev(X.payload(N, items, i_off, i_size))
    sym = torch.full((o_size + 16,), X.FILL, dtype=torch.uint8, device=dev)
    prf = torch.full((total * L * 32 + 16,), X.FILL, dtype=torch.uint8, device=dev)
    nodes = torch.full((3 * nn * 32 + 16,), X.FILL, dtype=torch.uint8, device=dev)
    c = gpu.SliverChecker(N)
    lib = _lib.lib()
    BUILD, CACHED = _lib.RS2_TREES_BUILD, _lib.RS2_TREES_CACHED
    u8, u16, u32, u64 = ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64
    ax = (u8 * 3)(*[X.AXES.index(it[0]) for it in items])
    sz = (u16 * 3)(*[it[1] for it in items])
    io, oo = (u64 * 3)(*i_off), (u64 * 3)(*o_off)
    counts = (u32 * 3)(*[len(it[3]) for it in items])
    flat = [t for it in items for t in it[3]]
    tg = (u16 * len(flat))(*flat)

    def call(handle=c.handle, m=3, a=ax, s=sz, sl=d_sl.data_ptr(), i=io, cnt=counts, t=tg,
             trees=BUILD, nd=nodes.data_ptr(), sy=sym.data_ptr(), o=oo, pr=prf.data_ptr()):
        return lib.rs2_sliver_checker_recovery_symbols_device_async(
            handle, m, ctypes.cast(a, ctypes.c_void_p) if a is not None else None, s, sl or None, i,
            cnt, t, trees, nd or None, sy or None, o, pr or None, None, None)

    big = 65536
    refused = {
        "null checker": call(handle=None),
        "null axis": call(a=None),
        "null sizes": call(s=None),
        "null d_slivers_base": call(sl=0),
        "null sliver_off": call(i=None),
        "null counts": call(cnt=None),
        "null targets": call(t=None),
        "null d_symbols_base": call(sy=0),
        "null symbols_off": call(o=None),
        "null d_proofs": call(pr=0),
        "trees = 2": call(trees=2),
        "trees = -1": call(trees=-1),
        "cached without nodes": call(trees=CACHED, nd=0),
        "odd d_slivers_base": call(sl=d_sl.data_ptr() + 1),
        "odd d_symbols_base": call(sy=sym.data_ptr() + 1),
        "d_proofs off 16": call(pr=prf.data_ptr() + 8),
        "d_nodes off 16": call(nd=nodes.data_ptr() + 2),
        "65536 slivers": call(m=big, a=(u8 * big)(), s=(u16 * big)(), i=(u64 * big)(),
                              cnt=(u32 * big)(), o=(u64 * big)()),
        "2^31 requests": call(m=2, cnt=(u32 * 2)(0x7FFFFFFF, 1)),
        "a 32-bit sum would wrap": call(m=2, cnt=(u32 * 2)(0x80000000, 0x80000000)),
    }
    for what, rc in refused.items():
        assert rc == X.INVALID, (what, rc)
    before = X.stats()
    assert call(m=0) == 0
    assert call(m=0, a=None, s=None, sl=0, i=None, cnt=None, t=None, sy=0, o=None, pr=0, nd=0) == 0
    assert X.moved(before) == [0] * 6
    torch.cuda.synchronize()
    for name, buf in (("d_symbols", sym), ("d_proofs", prf), ("d_nodes", nodes)):
        assert bool((buf == X.FILL).all()), name + " was written by a refused call"
    # all counts zero: the target list may be NULL, and the call warms the trees
    assert call(cnt=(u32 * 3)(), t=None) == 0, _lib.last_error()
    # and the accepted call still works on the same buffers
    assert call() == 0, _lib.last_error()
    torch.cuda.synchronize()
    X.check_outputs(N, items, sym.cpu().numpy()[:o_size], o_off, prf.cpu().numpy()[:total * L * 32],
                    nodes.cpu().numpy()[:3 * nn * 32], what="accepted")
    assert bool((sym[o_size:] == X.FILL).all()) and bool((prf[total * L * 32:] == X.FILL).all())
