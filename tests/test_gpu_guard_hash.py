"""The device hashing entry points inside guard bands: rs2_leaf_hashes_device_async,
rs2_merkle_roots_device_async, rs2_blob_id_device_async, SliverVerifier.roots_async and
recovery_symbols_async.  The leaf-hash and Merkle-root bodies are written against the `ops`
interface of walrus_amd/partition.py (leaf_hashes, merkle_roots) and run twice: on
tests/cpu_ops.CpuOps (unmarked; validates the layouts and the test logic on CPU tensors, one
placement) and on DeviceOps (-m gpu).

Every buffer has exactly its documented extent and lies in the interior of a
tests/guarded.Guarded allocation.  Symbol-carrying buffers are placed at each even residue
`delta` mod 16 (the leaf kernels align every symbol run down to 16 / 4 bytes and pick their
byte shifts from the residue); digest, proof and node buffers stay 16-byte aligned, as
include/walrus_rs2.h requires.  For every case and placement:

  A  containment   the output's guards and stride gaps keep their pattern
  B  independence  another fill of the inputs' guards (and stride gaps) gives bit-identical
                   outputs
  C  correctness   outputs equal hashlib.blake2b / rs2_oracle.merkle_* (merkle.rs:216-332)
"""
import hashlib

import numpy as np
import pytest
import torch

import rs2_oracle as O
from guarded import DELTAS, Guarded, ops_backend, strided_mask, sync

BACKENDS = ["cpu", pytest.param("device", marks=pytest.mark.gpu)]
CPU_DELTAS = (6,)

# both leaf kernels (one-block messages s <= 126, LDS windows above), each side of the 126 / 128
# switch and every 128-byte Blake2b block edge (message = 0x00 || symbol: s = 127 + 128 j)
LEAF_SIZES = [2, 4, 6, 14, 16, 18, 30, 32, 62, 64, 66, 124, 126, 128, 130, 254, 256, 258, 384,
              1024, 1150, 65534]
LEAF_COUNTS = (1, 63, 64, 65, 257)     # below / at / past one wave, past one 256-lane tile


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, device=None):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True).reshape(-1)).to(device or _dev())


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("s", LEAF_SIZES)
def test_leaf_hashes_guarded(request, name, s):
    ops, device = ops_backend(name, request)
    counts = (3,) if s == 65534 else LEAF_COUNTS
    rng = np.random.default_rng(s)
    syms = rng.integers(0, 256, (max(counts), s), dtype=np.uint8)
    ref = np.stack([np.frombuffer(hashlib.blake2b(b"\x00" + syms[i].tobytes(),
                                                  digest_size=32).digest(), dtype=np.uint8)
                    for i in range(max(counts))])
    for count in counts:
        data, want = _t(syms[:count], device), _t(ref[:count], device)
        for delta in (CPU_DELTAS if name == "cpu" else DELTAS):
            what = f"leaf hashes s={s} count={count} delta={delta}"
            outs = []
            for fill in (17, 201):
                src = Guarded(count * s, delta, device, fill).set(data)
                before = src.buf.clone()
                out = Guarded(count * 32, 0, device, fill=90)
                ops.leaf_hashes(src.payload, count, s, out.payload)
                sync(device)
                out.assert_guards_intact(None, what)                        # A
                assert torch.equal(src.buf, before), what + ": input written"
                assert torch.equal(out.payload, want), what                 # C
                outs.append(out.buf)
            assert torch.equal(outs[0], outs[1]), what + ": depends on bytes outside the input"  # B


# (n_trees, n_leaves, leaf_stride, tree_stride or None = leaves back to back, root_stride)
MERKLE_CASES = [
    (1, 1, 32, None, 32), (3, 2, 32, None, 48), (5, 3, 48, None, 64), (4, 10, 32, None, 32),
    (65, 7, 48, None, 48), (7, 100, 32, None, 64), (3, 100, 48, None, 32),
    (2, 1000, 32, None, 48), (3, 1000, 48, None, 64),
    (6, 10, 6 * 32, 32, 48),          # trees interleaved leaf by leaf (the partitioned encode)
    (5, 100, 5 * 32 + 16, 32, 32),
    (3, 10, 32, 10 * 32 + 16, 64),    # a gap between trees
    (2, 5000, 32, None, 48),          # above 4,096 leaves: the first levels fold through scratch
]


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("n_trees,n_leaves,leaf_stride,tree_stride,root_stride", MERKLE_CASES)
def test_merkle_roots_guarded(request, name, n_trees, n_leaves, leaf_stride, tree_stride,
                              root_stride):
    ops, device = ops_backend(name, request)
    if tree_stride is None:
        tree_stride = n_leaves * leaf_stride
    rng = np.random.default_rng(n_trees * 1000 + n_leaves)
    leaves = rng.integers(0, 256, (n_trees, n_leaves, 32), dtype=np.uint8)
    ref = np.stack([np.frombuffer(O.merkle_root_from_leaf_hashes(
        [leaves[t, i].tobytes() for i in range(n_leaves)]), dtype=np.uint8) for t in range(n_trees)])
    grid = (np.arange(n_trees)[:, None, None] * tree_stride +
            np.arange(n_leaves)[None, :, None] * leaf_stride + np.arange(32)[None, None, :])
    in_size = int(grid.max()) + 1
    out_size = (n_trees - 1) * root_stride + 32
    omask = strided_mask(out_size, n_trees, root_stride, 1, 32, 32)
    ogrid = torch.from_numpy(np.flatnonzero(omask)).to(device)
    lgrid = torch.from_numpy(grid.reshape(-1)).to(device)
    lvals, want = _t(leaves, device), _t(ref, device)
    what = f"merkle roots {n_trees}x{n_leaves} strides {leaf_stride}/{tree_stride}/{root_stride}"
    outs = []
    for fill in (17, 201):
        src = Guarded(in_size, 0, device, fill)
        src.payload[lgrid] = lvals
        before = src.buf.clone()
        out = Guarded(out_size, 0, device, fill=90)
        ops.merkle_roots(src.payload, n_trees, n_leaves, tree_stride, leaf_stride, out.payload,
                         root_stride)
        sync(device)
        out.assert_guards_intact(omask, what)                               # A
        assert torch.equal(src.buf, before), what + ": input written"
        assert torch.equal(out.payload[ogrid], want), what                  # C
        outs.append(out.buf)
    assert torch.equal(outs[0], outs[1]), what + ": depends on bytes outside the input"  # B


@pytest.mark.gpu
@pytest.mark.parametrize("n", [10, 100])
def test_blob_id_guarded(gpu, n):
    import ctypes
    from walrus_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    hashes = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    for blob_len in (0, 1, 123_457, (1 << 40) + 3):
        pairs = [(hashes[i, :32].tobytes(), hashes[i, 32:].tobytes()) for i in range(n)]
        want = _t(np.frombuffer(O.blob_id(pairs, blob_len), dtype=np.uint8))
        what = f"blob id n={n} blob_len={blob_len}"
        outs = []
        for fill in (17, 201):
            src = Guarded(n * 64, 0, _dev(), fill).set(hashes)
            before = src.buf.clone()
            out = Guarded(32, 0, _dev(), fill=90)
            assert L.rs2_blob_id_device_async(src.ptr, n, blob_len, out.ptr,
                                              ctypes.c_void_p(_stream())) == 0, what
            torch.cuda.synchronize()
            out.assert_guards_intact(None, what)                            # A
            assert torch.equal(src.buf, before), what + ": input written"
            assert torch.equal(out.payload, want), what                     # C
            outs.append(out.buf)
        assert torch.equal(outs[0], outs[1]), what                          # B


_VREF = {}


def _verifier_ref(n, s, axis, count):
    """`count` slivers of `axis` (K symbols each, K = the orthogonal code's source symbols), their
    n expanded symbols, Merkle roots and node arrays, from the oracle (shared by both tests)."""
    key = (n, s, axis, count)
    if key not in _VREF:
        kp, ks = O.source_symbols_for_n_shards(n)
        k = ks if axis == "primary" else kp
        rng = np.random.default_rng(n * 100 + s + (axis == "primary"))
        slivers = rng.integers(0, 256, (count, k, s), dtype=np.uint8)
        expanded = np.stack([O.rs_encode_all(slivers[i], n) for i in range(count)])
        leaf_data = [[expanded[i, j].tobytes() for j in range(n)] for i in range(count)]
        roots = np.stack([np.frombuffer(O.merkle_root(ld), dtype=np.uint8) for ld in leaf_data])
        nodes = np.stack([np.frombuffer(b"".join(O.merkle_nodes(ld)), dtype=np.uint8)
                          for ld in leaf_data])
        _VREF[key] = (slivers, expanded, leaf_data, roots, nodes)
    return _VREF[key]


VERIFIER_SHAPES = [(n, s, axis) for n in (10, 100) for s in (2, 6, 66, 130)
                   for axis in ("primary", "secondary")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,s,axis", VERIFIER_SHAPES)
def test_verifier_roots_guarded(gpu, n, s, axis):
    count = 3
    slivers, _, _, roots, _ = _verifier_ref(n, s, axis, count)
    v = gpu.encoding.SliverVerifier(n, s, axis)
    data, want = _t(slivers), _t(roots)
    for delta in DELTAS:
        what = f"verifier roots n={n} s={s} {axis} delta={delta}"
        outs = []
        for fill in (17, 201):
            src = Guarded(slivers.size, delta, _dev(), fill).set(data)
            before = src.buf.clone()
            out = Guarded(count * 32, 0, _dev(), fill=90)
            v.roots_async(count, src.ptr, out.ptr, _stream())
            torch.cuda.synchronize()
            out.assert_guards_intact(None, what)                            # A
            assert torch.equal(src.buf, before), what + ": input written"
            assert torch.equal(out.payload, want), what                     # C
            outs.append(out.buf)
        assert torch.equal(outs[0], outs[1]), what                          # B


@pytest.mark.gpu
@pytest.mark.parametrize("n,s,axis", VERIFIER_SHAPES)
def test_recovery_symbols_guarded(gpu, n, s, axis):
    import ctypes
    from walrus_amd import _lib
    count = 3
    slivers, expanded, leaf_data, _, nodes = _verifier_ref(n, s, axis, count)
    path_len, n_nodes = ctypes.c_uint32(), ctypes.c_uint64()
    assert _lib.lib().rs2_merkle_tree_shape(n, ctypes.byref(path_len), ctypes.byref(n_nodes)) == 0
    path_len, n_nodes = path_len.value, n_nodes.value
    assert nodes.shape == (count, n_nodes * 32)
    targets = [0, n - 1, n // 2]
    want_sym = _t(np.stack([expanded[i, t] for i, t in enumerate(targets)]))
    want_prf = _t(np.frombuffer(b"".join(b"".join(O.merkle_proof(leaf_data[i], t))
                                         for i, t in enumerate(targets)), dtype=np.uint8))
    assert want_prf.numel() == count * path_len * 32
    want_nodes = _t(nodes)
    v = gpu.encoding.SliverVerifier(n, s, axis)
    data = _t(slivers)
    for delta in DELTAS:
        for with_nodes in (True, False):
            what = f"recovery symbols n={n} s={s} {axis} delta={delta} nodes={with_nodes}"
            outs = []
            for fill in (17, 201):
                src = Guarded(slivers.size, delta, _dev(), fill).set(data)
                before = src.buf.clone()
                sym = Guarded(count * s, (delta + 6) % 16, _dev(), fill=90)
                prf = Guarded(count * path_len * 32, 0, _dev(), fill=91)
                nod = Guarded(count * n_nodes * 32, 0, _dev(), fill=92)
                v.recovery_symbols_async(count, src.ptr, targets, sym.ptr, prf.ptr,
                                         nod.ptr if with_nodes else 0, _stream())
                torch.cuda.synchronize()
                sym.assert_guards_intact(None, what + ": d_symbols")        # A
                prf.assert_guards_intact(None, what + ": d_proofs")
                nod.assert_guards_intact(None if with_nodes else [], what + ": d_nodes")
                assert torch.equal(src.buf, before), what + ": input written"
                assert torch.equal(sym.payload, want_sym), what             # C
                assert torch.equal(prf.payload, want_prf), what
                if with_nodes:
                    assert torch.equal(nod.payload, want_nodes), what
                outs.append(torch.cat([sym.buf, prf.buf, nod.buf]))
            assert torch.equal(outs[0], outs[1]), what                      # B


@pytest.mark.gpu
def test_hash_calls_reject_misaligned_pointers(gpu):
    """include/walrus_rs2.h: symbols 2-byte aligned; digest, proof and node buffers and the
    Merkle strides 16-byte aligned.  A violation is RS2_E_INVALID_ARGUMENT on the host and
    nothing is enqueued: the buffers stay as they were."""
    import ctypes
    from walrus_amd import _lib
    L = _lib.lib()
    INVALID = _lib.RS2_E_INVALID_ARGUMENT
    buf = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=_dev())
    a, b, c, d = (buf.data_ptr() + i * 16384 for i in range(4))
    st = ctypes.c_void_p(_stream())
    assert a % 16 == 0
    rcs = [L.rs2_leaf_hashes_device_async(a + 1, 4, 6, b, st)]
    rcs += [L.rs2_leaf_hashes_device_async(a, 4, 6, b + x, st) for x in (2, 4, 8)]
    for x in (2, 4, 8):
        rcs += [L.rs2_merkle_roots_device_async(a + x, 2, 4, 128, 32, b, 32, st),
                L.rs2_merkle_roots_device_async(a, 2, 4, 128, 32, b + x, 32, st),
                L.rs2_merkle_roots_device_async(a, 2, 4, 128 + x, 32, b, 32, st),
                L.rs2_merkle_roots_device_async(a, 2, 4, 256, 32 + x, b, 32, st),
                L.rs2_merkle_roots_device_async(a, 2, 4, 128, 32, b, 32 + x, st),
                L.rs2_blob_id_device_async(a + x, 4, 99, b, st),
                L.rs2_blob_id_device_async(a, 4, 99, b + x, st)]
    assert rcs == [INVALID] * len(rcs), rcs
    n, s = 10, 6
    v = gpu.encoding.SliverVerifier(n, s, "primary")
    with pytest.raises(ValueError, match="d_slivers must be 2-byte aligned"):
        v.roots_async(2, a + 1, b, _stream())
    with pytest.raises(ValueError, match="d_slivers must be 2-byte aligned"):
        v.recovery_symbols_async(2, a + 1, [0, 1], b, c, d, _stream())
    with pytest.raises(ValueError, match="d_symbols must be 2-byte aligned"):
        v.recovery_symbols_async(2, a, [0, 1], b + 1, c, d, _stream())
    for x in (2, 4, 8):
        with pytest.raises(ValueError, match="d_roots must be 16-byte aligned"):
            v.roots_async(2, a, b + x, _stream())
        with pytest.raises(ValueError, match="d_proofs must be 16-byte aligned"):
            v.recovery_symbols_async(2, a, [0, 1], b, c + x, d, _stream())
        with pytest.raises(ValueError, match="d_nodes must be 16-byte aligned"):
            v.recovery_symbols_async(2, a, [0, 1], b, c, d + x, _stream())
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()), "a refused call wrote to its buffers"
