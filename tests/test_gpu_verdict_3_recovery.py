"""Recovery-symbol proofs, sliver recovery and inconsistency proofs under corruption, against
the oracle (rs2_oracle.merkle_proof_root / recover_sliver / sliver_merkle_root).

  compute_roots on batches that mix honest entries with entries whose data, proof node or leaf
  index was changed: every root is the oracle's root of the entry as corrupted, and
  RecoverySymbol.verify raises for exactly those entries.
  One corrupted symbol among the "verified" ones: an InconsistencyProof comes back, and it does
  not verify against the honest metadata; the same symbol behind the ones that are used is
  never pulled.
  A blob that really is inconsistent (one source symbol replaced, the hashes of the sliver that
  carries it recomputed): the proof verifies against that metadata and fails against the
  honest one.
Each of them between honest calls on the same config.
"""
from itertools import cycle

import numpy as np
import pytest

import corruption as C
import rs2_oracle as O

pytestmark = pytest.mark.gpu

GEOS = ["G1", "G3", "G4"]
ORTH = {C.PRIMARY: C.SECONDARY, C.SECONDARY: C.PRIMARY}


def _sliver(gpu, sc, axis, index, data=None):
    return gpu.SliverData(gpu.Symbols(data if data is not None else sc.sliver(axis, index),
                                      sc.geo.symbol_size), index, axis)


def _target_pair(n, axis, target_sliver):
    return target_sliver if axis == C.PRIMARY else n - 1 - target_sliver


def _flip(data: bytes, byte: int, mask: int) -> bytes:
    d = bytearray(data)
    d[byte] ^= mask
    return bytes(d)


@pytest.mark.parametrize("gid", GEOS)
def test_compute_roots_mixed_batch(gpu, gid):
    from walrus_amd.recovery import MerkleProof, RecoverySymbol, compute_roots
    sc = C.scenario(gid)
    g, p = sc.geo, sc.params
    n, s = g.n, g.symbol_size
    cfg = gpu.ReedSolomonEncodingConfig(n)
    md = gpu.BlobMetadata(sc.hashes, g.length)
    L = gpu.recovery.path_length(n)
    # requests: sources of both axes, targets over the tree (first, last, odd, even leaves)
    sources, targets = [], []
    for j in range(24):
        axis = (C.PRIMARY, C.SECONDARY)[j % 2]
        sources.append(_sliver(gpu, sc, axis, (5 * j + 1) % n))
        targets.append((0, n - 1, n // 2, 3, n - 2, 1)[j % 6] if j < 12 else (7 * j) % n)
    syms = gpu.recovery_symbols_for_requests(cfg, sources, [
        _target_pair(n, ORTH[sl.axis], t) for sl, t in zip(sources, targets)])
    for sl, t, rs in zip(sources, targets, syms):
        exp = O.recovery_symbols(np.frombuffer(sl.symbols.data, np.uint8), sl.axis, p)
        leaves = [exp[i].tobytes() for i in range(n)]
        assert rs.axis == ORTH[sl.axis] and rs.index == sl.index
        assert rs.data == leaves[t] and rs.proof.path == O.merkle_proof(leaves, t)
        assert len(rs.proof.path) == L

    offs = cycle(C.symbol_offsets(s))
    mask = cycle((0x01, 0x80))
    level = cycle(range(L))
    node_byte = cycle((0, 31))

    def corrupt(kind, rs, t):
        """(symbol, leaf index) of the entry as corrupted."""
        if kind == "data":
            return RecoverySymbol(rs.axis, rs.index, _flip(rs.data, next(offs), next(mask)),
                                  rs.proof), t
        if kind == "node":
            path = list(rs.proof.path)
            lv = next(level)
            path[lv] = _flip(path[lv], next(node_byte), next(mask))
            return RecoverySymbol(rs.axis, rs.index, rs.data, MerkleProof(path)), t
        if kind == "sibling":
            return rs, t ^ 1
        return rs, n - 1

    def batch(which):
        """Entries [(symbol, leaf index, corrupted?)]: `which` maps entry -> kind."""
        out = []
        for j, (rs, t) in enumerate(zip(syms, targets)):
            kind = which.get(j)
            if kind == "sibling" and (t ^ 1) >= n or kind == "last" and t == n - 1:
                kind = "data"
            out.append(corrupt(kind, rs, t) + (kind is not None,) if kind else (rs, t, False))
        return out

    def check(entries):
        got = compute_roots([e[0].proof for e in entries], [e[0].data for e in entries],
                            [e[1] for e in entries])
        for j, (rs, t, bad) in enumerate(entries):
            want = O.merkle_proof_root(rs.proof.path, rs.data, t)
            assert got[j] == want, (gid, j, t, bad)
            honest_root = sc.hashes[sc.pair_of(ORTH[rs.axis], rs.index)][rs.axis == C.PRIMARY]
            assert (want != honest_root) == bad, (gid, j, t, bad)
            if bad:
                with pytest.raises(gpu.recovery.SymbolVerificationError) as e:
                    rs.verify(n, s, md, t)
                assert e.value.kind == "InvalidProof"
            else:
                rs.verify(n, s, md, t)

    kinds = ("data", "node", "sibling", "last")
    first = {j: kinds[(j // 2) % 4] for j in range(0, 24, 2)}        # every second entry
    first.update({0: "data", 23: "node"})                            # first and last of the batch
    levels = {j: "node" for j in range(1, 1 + 2 * L, 2)}             # a node at every path level
    second = {j: kinds[(j + 1) % 4] for j in range(1, 24, 3)}
    for which in ({}, first, {}, levels, second, {}):
        check(batch(which))


def _recovery_setup(gpu, sc, cfg, axis, target, extra=2, altered=None):
    """Recovery symbols for sliver `target` of `axis` from need + extra source slivers of the
    orthogonal axis (systematic and repair ones mixed); `altered` replaces source slivers."""
    n = sc.geo.n
    need = cfg.n_symbols_for_recovery(axis)
    src_idx = [(3 * j + 1) % n for j in range(need + extra)]
    assert len(set(src_idx)) == len(src_idx)
    altered = altered or {}
    sources = [_sliver(gpu, sc, ORTH[axis], i, altered.get(i)) for i in src_idx]
    syms = gpu.recovery_symbols_for_requests(cfg, sources,
                                             [_target_pair(n, axis, target)] * len(sources))
    return need, src_idx, syms


@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", GEOS)
def test_one_corrupt_symbol(gpu, gid, axis):
    R = gpu.recovery
    sc = C.scenario(gid)
    g = sc.geo
    cfg = gpu.ReedSolomonEncodingConfig(g.n)
    md = gpu.BlobMetadata(sc.hashes, g.length)
    target = 2
    need, _, syms = _recovery_setup(gpu, sc, cfg, axis, target)
    want = sc.sliver(axis, target)

    def honest():
        got = gpu.recover_sliver_or_generate_inconsistency_proof(syms, target, md, cfg, axis)
        assert isinstance(got, gpu.SliverData) and got.symbols.data == want
        assert got.index == target and got.axis == axis

    honest()
    positions = [(0, 0x01), (g.symbol_size - 1, 0x80)] + \
        [(o, 0x01) for o in C.symbol_offsets(g.symbol_size)[1:-1]]
    members = cycle((0, need - 1, need // 2))
    for k, (byte, mask) in enumerate(positions):
        m = next(members)
        bad = list(syms)
        bad[m] = R.RecoverySymbol(syms[m].axis, syms[m].index, _flip(syms[m].data, byte, mask),
                                  syms[m].proof)
        proof = gpu.recover_sliver_or_generate_inconsistency_proof(bad, target, md, cfg, axis)
        assert isinstance(proof, gpu.InconsistencyProof), (gid, axis, m, byte)
        assert proof.axis == axis and proof.target_sliver_index == target
        assert proof.recovery_symbols == bad[:need]
        with pytest.raises(R.InconsistencyVerificationError) as e:
            proof.verify(md, cfg)
        assert e.value.kind == "InvalidRecoverySymbols"
        # the decode behind it is the oracle's decode of the symbols as corrupted
        dec = gpu.SliverData.recover_sliver_from_decoding_symbols(
            [r.into_decoding_symbol() for r in bad[:need]], target, g.symbol_size, cfg, axis)
        ref = O.recover_sliver(axis, [(r.index, np.frombuffer(r.data, np.uint8))
                                      for r in bad[:need]], sc.params)
        assert dec.symbols.data == ref.tobytes() != want
        # the same symbol behind the first `need`: never pulled
        late = list(syms)
        late[need + k % 2] = R.RecoverySymbol(syms[need].axis, syms[need + k % 2].index,
                                              _flip(syms[need + k % 2].data, byte, mask),
                                              syms[need + k % 2].proof)
        got = gpu.recover_sliver_or_generate_inconsistency_proof(late, target, md, cfg, axis)
        assert isinstance(got, gpu.SliverData) and got.symbols.data == want
        if k % 2:
            honest()
    honest()


@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
@pytest.mark.parametrize("gid", GEOS)
def test_inconsistent_blob(gpu, gid, axis):
    """Source symbol (target, c0) of the matrix replaced in the one source sliver that carries
    it (sliver c0 of the orthogonal axis, whose symbol `target` it is), that sliver's hash
    recomputed with the oracle: every recovery symbol verifies against this metadata, the
    recovered sliver contradicts its own hash, so the proof holds -- and fails against the
    honest metadata, where the altered symbol has no valid proof."""
    R = gpu.recovery
    sc = C.scenario(gid)
    g, p = sc.geo, sc.params
    n, s = g.n, g.symbol_size
    cfg = gpu.ReedSolomonEncodingConfig(n)
    md = gpu.BlobMetadata(sc.hashes, g.length)
    orth = ORTH[axis]
    target = 1                                   # a systematic sliver: its symbols are sources
    need, src_idx, honest_syms = _recovery_setup(gpu, sc, cfg, axis, target, extra=0)
    want = sc.sliver(axis, target)

    def honest():
        got = gpu.recover_sliver_or_generate_inconsistency_proof(honest_syms, target, md, cfg,
                                                                 axis)
        assert isinstance(got, gpu.SliverData) and got.symbols.data == want

    honest()
    k_orth = p.n_primary if orth == C.SECONDARY else p.n_secondary   # symbols per source sliver
    assert target < k_orth
    for c0, (off, mask) in zip((src_idx[0], src_idx[-1], src_idx[need // 2]),
                               ((0, 0x01), (s - 1, 0x80), (s // 2, 0x01))):
        data = _flip(sc.sliver(orth, c0), target * s + off, mask)
        hashes = list(sc.hashes)
        pair = sc.pair_of(orth, c0)
        root = C.sliver_root(p, orth, data)
        hashes[pair] = (root, hashes[pair][1]) if orth == C.PRIMARY else (hashes[pair][0], root)
        md_bad = gpu.BlobMetadata(hashes, g.length)
        _, _, syms = _recovery_setup(gpu, sc, cfg, axis, target, extra=0, altered={c0: data})
        for r in syms:                            # every proof verifies
            r.verify(n, s, md_bad, target)
        ref = O.recover_sliver(axis, [(r.index, np.frombuffer(r.data, np.uint8)) for r in syms],
                               p).tobytes()
        assert ref != want and C.sliver_root(p, axis, ref) != \
            sc.hashes[sc.pair_of(axis, target)][axis == C.SECONDARY]
        proof = gpu.recover_sliver_or_generate_inconsistency_proof(syms, target, md_bad, cfg, axis)
        assert isinstance(proof, gpu.InconsistencyProof), (gid, axis, c0)
        proof.verify(md_bad, cfg)
        with pytest.raises(R.InconsistencyVerificationError) as e:
            proof.verify(md, cfg)
        assert e.value.kind == "InvalidRecoverySymbols"
        honest()
