"""Helpers of the bulk recovery-symbol tests (tests/test_gpu_symbols_multi_*.py) -- TEST ONLY, a
plain module.  References come from rs2_oracle (O.recovery_symbols, O.merkle_nodes,
O.merkle_proof) for bare random slivers, and for n above 4,096 from the C restatement
(rs2cpu_encode_1d, rs2cpu_recovery_symbol); each is computed once per key, shared and left
unchanged.  `run` issues one rs2_verifier_recovery_symbols_multi_device_async call on torch
buffers and returns what it wrote; `run_single` the existing per-request call with the source
sliver repeated once per target (the independent cross-check)."""
import ctypes

import numpy as np
import torch

import rs2_oracle as O
from walrus_amd import _lib

AXES = ("primary", "secondary")
FILL = 0xEE            # outputs hold this before a call
INVALID = _lib.RS2_E_INVALID_ARGUMENT


def k_of(n, axis):
    """Symbols of a sliver of `axis`: K_s for a primary sliver, K_p for a secondary one."""
    kp, ks = O.source_symbols_for_n_shards(n)
    return ks if axis == "primary" else kp


def shape(n):
    """(path_len, n_nodes) of a tree over n leaves (rs2_merkle_tree_shape; device free)."""
    path_len, n_nodes = ctypes.c_uint32(), ctypes.c_uint64()
    assert _lib.lib().rs2_merkle_tree_shape(n, ctypes.byref(path_len), ctypes.byref(n_nodes)) == 0
    return path_len.value, n_nodes.value


def stats():
    out = (ctypes.c_uint64 * 5)()
    assert _lib.lib().rs2_recovery_symbols_stats(out) == 0
    return [int(x) for x in out]


def moved(before):
    return [a - b for a, b in zip(stats(), before)]


_REF = {}


def reference(n, s, axis, count, seed=0, cpu=None):
    """`count` random bare slivers of `axis`: data (count, k*s), expanded (count, n, s), leaf_data
    and nodes (count, n_nodes*32).  cpu: the C restatement, used for the expansion instead of the
    Python oracle (n above 4,096)."""
    key = (n, s, axis, count, seed, cpu is not None)
    if key not in _REF:
        k = k_of(n, axis)
        p = O.Rs2Params(n, *O.source_symbols_for_n_shards(n), s, 0)
        rng = np.random.default_rng([n, s, AXES.index(axis), seed, 77])
        data = rng.integers(0, 256, (count, k * s), dtype=np.uint8)
        if cpu is None:
            expanded = np.stack([O.recovery_symbols(data[i], axis, p) for i in range(count)])
        else:
            expanded = np.zeros((count, n, s), dtype=np.uint8)
            cpu.rs2cpu_encode_1d.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p] * 2
            assert cpu.rs2cpu_encode_1d(k, n, s, count, data.ctypes.data, expanded.ctypes.data) == 0
        leaf_data = [[expanded[i, j].tobytes() for j in range(n)] for i in range(count)]
        nodes = np.stack([np.frombuffer(b"".join(O.merkle_nodes(ld)), dtype=np.uint8)
                          for ld in leaf_data])
        for a in (data, expanded, nodes):
            a.setflags(write=False)
        _REF[key] = {"n": n, "s": s, "axis": axis, "k": k, "data": data, "expanded": expanded,
                     "leaf_data": leaf_data, "nodes": nodes, "proofs": {}}
    return _REF[key]


def expected(ref, targets):
    """(symbols, proofs) the call must write for targets[i] of sliver i, request after request:
    the expanded symbol and O.merkle_proof of the target's leaf."""
    L = shape(ref["n"])[0]
    sym, prf = [], []
    for i, ts in enumerate(targets):
        for t in ts:
            if (i, t) not in ref["proofs"]:
                path = O.merkle_proof(ref["leaf_data"][i], t)
                assert len(path) == L
                ref["proofs"][(i, t)] = b"".join(path)
            sym.append(ref["expanded"][i, t].tobytes())
            prf.append(ref["proofs"][(i, t)])
    return (np.frombuffer(b"".join(sym), dtype=np.uint8),
            np.frombuffer(b"".join(prf), dtype=np.uint8))


def dev():
    return torch.device("cuda", 0)


def to_dev(a):
    return torch.tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.uint8, device=dev())


def run(v, ref, targets, trees="build", nodes=None, want_nodes=False, stream=None, slivers=None):
    """One bulk call on verifier v.  nodes: a device tensor holding the trees (CACHED, or BUILD
    into it); want_nodes: BUILD into a fresh filled buffer.  Returns (rc, symbols, proofs, nodes)
    as numpy arrays after a device synchronize (nodes None when the call had none)."""
    n, s = ref["n"], ref["s"]
    L, nn = shape(n)
    m = len(targets)
    total = sum(len(t) for t in targets)
    d_sl = to_dev(ref["data"][:m]) if slivers is None else slivers
    d_sym = torch.full((max(total * s, 2),), FILL, dtype=torch.uint8, device=dev())
    d_prf = torch.full((max(total * L * 32, 32),), FILL, dtype=torch.uint8, device=dev())
    if nodes is None and want_nodes:
        nodes = torch.full((m * nn * 32,), FILL, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    rc = v.recovery_symbols_multi_async(d_sl.data_ptr(), targets, d_sym.data_ptr(),
                                        d_prf.data_ptr(), nodes.data_ptr() if nodes is not None
                                        else 0, trees, stream)
    torch.cuda.synchronize()
    return (rc, d_sym.cpu().numpy()[:total * s], d_prf.cpu().numpy()[:total * L * 32],
            None if nodes is None else nodes.cpu().numpy())


def run_single(v, ref, targets):
    """The same requests through rs2_verifier_recovery_symbols_device_async: request j passes its
    source sliver again."""
    n, s = ref["n"], ref["s"]
    L, _ = shape(n)
    flat = [(i, t) for i, ts in enumerate(targets) for t in ts]
    d_sl = to_dev(np.stack([ref["data"][i] for i, _ in flat]))
    d_sym = torch.full((len(flat) * s,), FILL, dtype=torch.uint8, device=dev())
    d_prf = torch.full((max(len(flat) * L * 32, 32),), FILL, dtype=torch.uint8, device=dev())
    v.recovery_symbols_async(len(flat), d_sl.data_ptr(), [t for _, t in flat], d_sym.data_ptr(),
                             d_prf.data_ptr())
    torch.cuda.synchronize()
    return d_sym.cpu().numpy(), d_prf.cpu().numpy()[:len(flat) * L * 32]


def check(v, ref, targets, trees="build", nodes=None, want_nodes=False, single=True):
    """A bulk call whose every symbol and proof byte equals the oracle's (and, with `single`, the
    per-request call's); with want_nodes the trees equal O.merkle_nodes.  Returns run()'s tuple."""
    rc, sym, prf, got_nodes = run(v, ref, targets, trees, nodes, want_nodes)
    assert rc == 0, _lib.last_error()
    want_sym, want_prf = expected(ref, targets)
    assert sym.tobytes() == want_sym.tobytes(), "symbols differ from the oracle's"
    assert prf.tobytes() == want_prf.tobytes(), "proofs differ from the oracle's"
    if want_nodes:
        assert got_nodes.tobytes() == ref["nodes"][:len(targets)].tobytes(), "trees differ"
    if single and sym.size:
        ssym, sprf = run_single(v, ref, targets)
        assert ssym.tobytes() == sym.tobytes() and sprf.tobytes() == prf.tobytes(), \
            "the bulk call and the per-request call disagree"
    return rc, sym, prf, got_nodes
