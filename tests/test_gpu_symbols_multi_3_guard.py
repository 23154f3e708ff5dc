"""rs2_verifier_recovery_symbols_multi_device_async inside guard bands (tests/guarded.py): every
buffer of both modes is the interior of a larger patterned allocation, d_slivers and d_symbols at
every even placement mod 16 (so the symbol copy takes each of its widths: 16-byte pieces when the
two are congruent mod 16, 4-byte pieces mod 4, else 2-byte pieces, with 2-byte edges), the proof
and node buffers 16-byte aligned.  Nothing outside the stated extents may change, CACHED leaves
d_nodes as it was, and a second run with another guard fill gives the same bytes: no result
depends on a byte outside an input's extent.  Then every refusal of the header returns its code
with the outputs' fill untouched."""
import ctypes

import numpy as np
import pytest
import torch

import symbols_multi as M
from guarded import DELTAS, Guarded
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 10


def _run(v, ref, targets, d_in, d_out, fill, trees, cached_nodes=None):
    dev = M.dev()
    s = ref["s"]
    L, nn = M.shape(N)
    m = len(targets)
    total = sum(len(t) for t in targets)
    data = np.array(ref["data"][:m]).reshape(-1)      # (a writable copy: the reference is not)
    slivers = Guarded(data.size, d_in, dev, fill).set(data)
    sym = Guarded(total * s, d_out, dev, 77)
    prf = Guarded(total * L * 32, 0, dev, 78)
    nodes = Guarded(m * nn * 32, 0, dev, fill + 2)
    if cached_nodes is not None:
        nodes.set(np.array(cached_nodes))
    torch.cuda.synchronize()
    rc = v.recovery_symbols_multi_async(slivers.ptr, targets, sym.ptr, prf.ptr, nodes.ptr, trees)
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    slivers.assert_guards_intact(what="d_slivers")
    assert slivers.numpy().tobytes() == data.tobytes(), "d_slivers was written"
    sym.assert_guards_intact(what="d_symbols")
    prf.assert_guards_intact(what="d_proofs")
    nodes.assert_guards_intact(what="d_nodes")
    return sym.numpy(), prf.numpy(), nodes.numpy()


@pytest.mark.parametrize("d_out", DELTAS)
@pytest.mark.parametrize("d_in", DELTAS)
@pytest.mark.parametrize("s", [2, 6, 18])
def test_inside_guards(gpu, s, d_in, d_out):
    for axis in M.AXES:
        k = M.k_of(N, axis)
        ref = M.reference(N, s, axis, 3)
        targets = [list(range(N)), [], [N - 1, k, k - 1, 0, k]]
        want_sym, want_prf = M.expected(ref, targets)
        want_nodes = ref["nodes"][:3].reshape(-1)
        v = gpu.SliverVerifier(N, s, axis)
        for fill in (11, 151):
            sym, prf, nodes = _run(v, ref, targets, d_in, d_out, fill, "build")
            assert sym.tobytes() == want_sym.tobytes(), (axis, fill)
            assert prf.tobytes() == want_prf.tobytes(), (axis, fill)
            assert nodes.tobytes() == want_nodes.tobytes(), (axis, fill)
            sym, prf, nodes = _run(v, ref, targets, d_in, d_out, fill, "cached", want_nodes)
            assert sym.tobytes() == want_sym.tobytes(), (axis, fill)
            assert prf.tobytes() == want_prf.tobytes(), (axis, fill)
            assert nodes.tobytes() == want_nodes.tobytes(), "a CACHED call wrote d_nodes"


def test_refusals_leave_outputs_untouched(gpu):
    s, axis = 6, "primary"
    ref = M.reference(N, s, axis, 3)
    L, nn = M.shape(N)
    dev = M.dev()
    slivers = M.to_dev(ref["data"][:3])
    sym = torch.full((64 * s + 16,), M.FILL, dtype=torch.uint8, device=dev)
    prf = torch.full((64 * L * 32 + 16,), M.FILL, dtype=torch.uint8, device=dev)
    nodes = torch.full((3 * nn * 32 + 16,), M.FILL, dtype=torch.uint8, device=dev)
    v = gpu.SliverVerifier(N, s, axis)
    lib = _lib.lib()
    BUILD, CACHED = _lib.RS2_TREES_BUILD, _lib.RS2_TREES_CACHED
    u32, u16 = ctypes.c_uint32, ctypes.c_uint16
    counts = (u32 * 3)(2, 0, 1)
    tg = (u16 * 3)(0, 9, 7)

    def call(handle=v.handle, m=3, sl=slivers.data_ptr(), cnt=counts, t=tg, trees=BUILD,
             nd=nodes.data_ptr(), sy=sym.data_ptr(), pr=prf.data_ptr()):
        return lib.rs2_verifier_recovery_symbols_multi_device_async(
            handle, m, sl or None, cnt, t, trees, nd or None, sy or None, pr or None, None)

    refused = {
        "null verifier": call(handle=None),
        "null d_slivers": call(sl=0),
        "null counts": call(cnt=None),
        "null targets": call(t=None),
        "null d_symbols": call(sy=0),
        "null d_proofs": call(pr=0),
        "trees = 2": call(trees=2),
        "trees = -1": call(trees=-1),
        "cached without nodes": call(trees=CACHED, nd=0),
        "odd d_slivers": call(sl=slivers.data_ptr() + 1),
        "odd d_symbols": call(sy=sym.data_ptr() + 1),
        "d_proofs off 16": call(pr=prf.data_ptr() + 8),
        "d_nodes off 16": call(nd=nodes.data_ptr() + 2),
        "d_nodes off 16, cached": call(trees=CACHED, nd=nodes.data_ptr() + 4),
        "65536 slivers": call(m=65536, cnt=(u32 * 65536)()),
        "target = n": call(t=(u16 * 3)(0, N, 7)),
        "target = 65535": call(t=(u16 * 3)(0, 9, 65535)),
        "2^31 requests": call(m=2, cnt=(u32 * 2)(0x7FFFFFFF, 1)),
        "a 32-bit sum would wrap": call(m=2, cnt=(u32 * 2)(0x80000000, 0x80000000)),
    }
    for what, rc in refused.items():
        assert rc == M.INVALID, (what, rc)
    before = M.stats()
    assert call(m=0) == 0 and call(m=0, sl=0, cnt=None, t=None, sy=0, pr=0, nd=0) == 0
    assert M.moved(before) == [0] * 5
    torch.cuda.synchronize()
    for name, buf in (("d_symbols", sym), ("d_proofs", prf), ("d_nodes", nodes)):
        assert bool((buf == M.FILL).all()), name + " was written by a refused call"
    # and the accepted call still works on the same buffers
    assert call() == 0, _lib.last_error()
    torch.cuda.synchronize()
    want_sym, want_prf = M.expected(ref, [[0, 9], [], [7]])
    assert sym[:3 * s].cpu().numpy().tobytes() == want_sym.tobytes()
    assert prf[:3 * L * 32].cpu().numpy().tobytes() == want_prf.tobytes()
    assert bool((sym[3 * s:] == M.FILL).all()) and bool((prf[3 * L * 32:] == M.FILL).all())
