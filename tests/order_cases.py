"""Shapes and CPU references of the stream-ordering tests (tests/test_gpu_order_*.py), device
free: the C restatement (golden/make_fullsize.load_cpu) for whole-blob encodes, rs2_oracle for
1D codewords and Merkle trees.  tests/test_stream_order_model.py checks the shape facts claimed
here on the CPU.  Every reference is computed once per key, shared, and left unchanged."""
import ctypes
import os
import sys

import numpy as np

import rs2_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_fullsize import blob_bytes, load_cpu  # noqa: E402

# (n_shards, blob length, symbol size): the single-blob encode shapes
#   tail rows + the one-block leaf kernel; the LDS-window leaf kernel (s > 126); the two
#   smallest messages of the >= 64 MiB graph, without and with a padded last row
ENCODE_SHAPES = [(10, 151, 6), (100, 300_000, 132), (100, 67_109_880, 29_460),
                 (100, 67_109_875, 29_460)]
SPLIT_SHAPES = [(100, 300_000, 132), (100, 67_109_875, 29_460)]
BIG_MESSAGE = 64 << 20
# (n_shards, symbol size, the 4 blob lengths) of the batch encodes
BATCH_SHAPES = [(10, 6, (168, 151, 130, 113)), (100, 14, (31_892, 31_001, 29_000, 27_337))]
DECODE_SHAPES = [(10, 151, 6), (100, 300_000, 132)]
DECODE_BATCH = (13, 40, (1800, 1799, 1750, 1733, 1711))
CODEC_SHAPES = [(5, 11, 130), (334, 1000, 6)]          # (k, n, s), 3 lines
VERIFIER_SHAPES = [(10, 6), (100, 130)]                # (n, s), both axes, count 3
DEPTH_DECODE = (100, 300_000, 132)


def symbol_size(n, length):
    kp, ks = O.source_symbols_for_n_shards(n)
    return O.compute_symbol_size(length, kp * ks)


_CPU = []


def cpu():
    if not _CPU:
        _CPU.append(load_cpu())
    return _CPU[0]


def c_params(n, length):
    kp, ks, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    cpu().rs2cpu_params(n, length, ctypes.byref(kp), ctypes.byref(ks), ctypes.byref(s))
    return kp.value, ks.value, s.value


def c_encode(n, blob):
    """rs2cpu_encode of `blob` (uint8 array): primary (n, K_s*s), secondary (n, K_p*s) by sliver
    index, the n pair hashes (n*64) and the BlobId (32)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    kp, ks, s = c_params(n, blob.size)
    prim = np.empty((n, ks * s), dtype=np.uint8)
    sec = np.empty((n, kp * s), dtype=np.uint8)
    hashes = np.empty(n * 64, dtype=np.uint8)
    bid = np.empty(32, dtype=np.uint8)
    cpu().rs2cpu_encode(n, blob.ctypes.data, blob.size, prim.ctypes.data, sec.ctypes.data,
                        hashes.ctypes.data, bid.ctypes.data)
    return {"blob": blob, "primary": prim, "secondary": sec, "hashes": hashes, "blob_id": bid,
            "kp": kp, "ks": ks, "s": s}


_ENC = {}


def encoded(n, length, seed=0):
    """The encode of blob_bytes(1000 + seed, length) at n shards; seed 0 is the real blob of a
    test, other seeds make its decoys (valid blobs / slivers of the same shape)."""
    key = (n, length, seed)
    if key not in _ENC:
        e = c_encode(n, blob_bytes(1000 + seed + 17 * n, length))
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ENC[key] = e
    return _ENC[key]


def decoy_blob(n, length, seed):
    a = blob_bytes(1000 + seed + 17 * n, length)
    a.setflags(write=False)
    return a


def k_of(n, axis):
    """Symbols of a sliver of `axis`: K_s for a primary sliver, K_p for a secondary one."""
    kp, ks = O.source_symbols_for_n_shards(n)
    return ks if axis == "primary" else kp


_SLV = {}


def slivers(n, s, axis, count, seed=0):
    """`count` random slivers of `axis` with what the verifier calls return for them, from the
    oracle: data (count, K, s), their n expanded symbols (count, n, s), roots (count, 32), node
    arrays (count, n_nodes*32) and the leaves' byte strings."""
    key = (n, s, axis, count, seed)
    if key not in _SLV:
        k = k_of(n, axis)
        rng = np.random.default_rng([n, s, int(axis == "primary"), seed])
        data = rng.integers(0, 256, (count, k, s), dtype=np.uint8)
        expanded = np.stack([O.rs_encode_all(data[i], n) for i in range(count)])
        leaf_data = [[expanded[i, j].tobytes() for j in range(n)] for i in range(count)]
        roots = np.stack([np.frombuffer(O.merkle_root(ld), dtype=np.uint8) for ld in leaf_data])
        nodes = np.stack([np.frombuffer(b"".join(O.merkle_nodes(ld)), dtype=np.uint8)
                          for ld in leaf_data])
        for a in (data, expanded, roots, nodes):
            a.setflags(write=False)
        _SLV[key] = {"data": data, "expanded": expanded, "leaf_data": leaf_data, "roots": roots,
                     "nodes": nodes}
    return _SLV[key]


def proofs(ref, targets):
    """Merkle paths of leaf targets[i] in sliver i's tree, back to back."""
    return np.frombuffer(b"".join(b"".join(O.merkle_proof(ref["leaf_data"][i], t))
                                  for i, t in enumerate(targets)), dtype=np.uint8)


_CW = {}


def codewords(k, n, s, lines, seed=0):
    """`lines` codewords of the (k, n) code, (lines, n, s) bytes, source || repair (oracle)."""
    key = (k, n, s, lines, seed)
    if key not in _CW:
        rng = np.random.default_rng([k, n, s, seed])
        data = rng.integers(0, 256, (lines, k, s), dtype=np.uint8)
        cw = np.stack([O.rs_encode_all(data[i], n) for i in range(lines)])
        cw.setflags(write=False)
        _CW[key] = cw
    return _CW[key]


def subset(n, k, seed):
    """A random k-subset of 0..n-1 in random order that leaves out index 0 (so at least one
    original is erased and the decode kernels run)."""
    rng = np.random.default_rng([n, k, seed])
    return [int(i) + 1 for i in rng.permutation(n - 1)[:k]]
