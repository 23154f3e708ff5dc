"""Batched sliver recovery on the device (rs2_verifier_recover_slivers_device_async /
rs2_recover_slivers), the proof check in front of it (rs2_verifier_check_recovery_symbols_device_
async / rs2_check_recovery_symbols) and the Python layer over both.

A sliver is one codeword of a 1D code, so most tests build their slivers straight from the oracle's
1D encoder (O.rs_encode_all: the sliver's n recovery symbols) and its Merkle tree; the small-shape
test goes through whole blobs and the engine's own recovery-symbol service instead.
rs2_recover_stats deltas pin which path each sliver took."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import rs2_oracle as O
from guarded import Guarded

pytestmark = pytest.mark.gpu

FILL = 7
OK, E_NOT_ENOUGH, E_UNSUCCESSFUL, E_INVALID = 0, -5, -6, -8
MISMATCH, MATCH, SKIPPED = 0, 1, 2
CHUNK_JOBS = 341  # jobs of one batched launch (an upload slot of 512 KiB / 1536-byte jobs)


def _stats():
    from walrus_amd.encoding import recover_stats
    s = recover_stats()
    return np.array([s["launches"], s["batched"], s["single"]], dtype=np.int64)


def _k(n, axis):
    """Symbols of a sliver of `axis`: K_s for a primary sliver, K_p for a secondary one."""
    kp, ks = O.source_symbols_for_n_shards(n)
    return ks if axis == "primary" else kp


class Sliver:
    """A random sliver of K symbols with its n recovery symbols and Merkle root (oracle)."""

    def __init__(self, n, K, s, rng):
        self.data = rng.integers(0, 256, (K, s), dtype=np.uint8)
        self.all = O.rs_encode_all(self.data, n)
        self.root = O.merkle_root([x.tobytes() for x in self.all])


def _subsets(n, K, count, rng):
    """all-repair (topped up with the last originals), all-original, one erasure, then random
    K-subsets that leave out original 0 -- in random order, a different one per sliver."""
    gone = int(rng.integers(K))
    subs = [list(range(n - 1, -1, -1))[:K], list(range(K)),
            [i for i in range(K) if i != gone] + [K + int(rng.integers(n - K))]]
    while len(subs) < count:
        subs.append([int(i) + 1 for i in rng.permutation(n - 1)[:K]])
    return subs[:count]


class Call:
    """One device call: symbols, outputs, roots and verdicts in guard bands."""

    def __init__(self, n, s, axis, lists, datas, expected, delta=0, in_fill=FILL, roots=True,
                 verdict=True):
        dev = torch.device("cuda", 0)
        self.n, self.s, self.K, self.m = n, s, _k(n, axis), len(lists)
        self.lists = lists
        flat = np.concatenate([np.asarray(d, dtype=np.uint8).reshape(-1) for d in datas]) \
            if sum(len(x) for x in lists) else np.zeros(0, dtype=np.uint8)
        self.flat = flat
        self.sym = Guarded(max(flat.size, 2), delta, dev, fill=in_fill).set(flat)
        self.out = Guarded(self.m * self.K * s, delta, dev, fill=FILL)
        self.roots = Guarded(self.m * 32, 0, dev, fill=FILL) if roots else None
        self.verdict = Guarded(self.m * 4, 0, dev, fill=FILL) if verdict else None
        self.expected = b"".join(expected) if expected is not None else None

    def run(self, verifier, statuses=False, stream=None):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return verifier.recover_slivers_async(
            self.lists, self.sym.ptr, self.out.ptr, self.expected,
            self.roots.ptr if self.roots else 0, self.verdict.ptr if self.verdict else 0, st,
            statuses)

    def results(self):
        torch.cuda.synchronize()
        out = self.out.numpy().reshape(self.m, self.K * self.s)
        roots = self.roots.numpy().reshape(self.m, 32) if self.roots else None
        verdict = self.verdict.numpy().view(np.int32) if self.verdict else None
        return out, roots, verdict

    def assert_guards(self):
        for g, what in ((self.sym, "d_symbols"), (self.out, "d_slivers_out"),
                        (self.roots, "d_roots"), (self.verdict, "d_verdict")):
            if g is not None:
                g.assert_guards_intact(what=what)
        assert np.array_equal(self.sym.numpy()[:self.flat.size], self.flat), "d_symbols written"


def _call_for(n, s, axis, slivers, subs, **kw):
    datas = [sl.all[sel] for sl, sel in zip(slivers, subs)]
    return Call(n, s, axis, subs, datas, [sl.root for sl in slivers], **kw)


def _check_exact(call, slivers, skipped=()):
    out, roots, verdict = call.results()
    pat_out = Guarded(call.out.size, call.out.delta, "cpu", fill=FILL).numpy().reshape(out.shape)
    pat_roots = Guarded(call.m * 32, 0, "cpu", fill=FILL).numpy().reshape(call.m, 32)
    for i, sl in enumerate(slivers):
        if i in skipped:
            assert np.array_equal(out[i], pat_out[i]), f"skipped sliver {i}: output written"
            if roots is not None:
                assert np.array_equal(roots[i], pat_roots[i]), f"skipped sliver {i}: root written"
            if verdict is not None:
                assert verdict[i] == SKIPPED
            continue
        assert np.array_equal(out[i], sl.data.reshape(-1)), f"sliver {i} differs"
        if roots is not None:
            assert roots[i].tobytes() == sl.root, f"root {i} differs"
        if verdict is not None:
            assert verdict[i] == MATCH, (i, verdict[i])
    call.assert_guards()


# ---- 1. small shapes through whole blobs: device and host forms -----------------------------
@pytest.mark.parametrize("n,s", [(10, 6), (10, 40), (13, 6), (13, 40)])
def test_small_shapes_device_and_host_forms(gpu, n, s):
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverVerifier
    rng = np.random.default_rng(n * 100 + s)
    kp, ks = O.source_symbols_for_n_shards(n)
    cfg = gpu.ReedSolomonEncodingConfig(n)
    blobs = [rng.integers(0, 256, s * kp * ks - b, dtype=np.uint8).tobytes() for b in range(3)]
    enc = [cfg.encode_with_metadata(b) for b in blobs]
    ref = [O.encode_with_metadata(b, n) for b in blobs]
    X = [O.expanded_matrix(b, r.params) for b, r in zip(blobs, ref)]
    for axis in ("primary", "secondary"):
        K = _k(n, axis)
        prim = axis == "primary"
        targets = [(b, int(t)) for b in range(3) for t in rng.permutation(n)[:3]]  # 9 slivers
        subs = _subsets(n, K, len(targets), rng)
        # the received symbols from the engine's recovery-symbol service, one request per symbol
        srcs, tps = [], []
        for (b, t), sel in zip(targets, subs):
            for q in sel:
                # source sliver q of the orthogonal axis, asked for target sliver t's pair
                pair = enc[b][0][n - 1 - q if prim else q]
                srcs.append(pair.secondary if prim else pair.primary)
                tps.append(t if prim else n - 1 - t)
        syms = gpu.recovery_symbols_for_requests(cfg, srcs, tps)
        datas, at = [], 0
        for (b, t), sel in zip(targets, subs):
            got = np.stack([np.frombuffer(syms[at + j].data, dtype=np.uint8)
                            for j in range(len(sel))])
            want = np.stack([X[b][t, q] if prim else X[b][q, t] for q in sel])
            assert np.array_equal(got, want)
            assert [syms[at + j].index for j in range(len(sel))] == sel
            datas.append(got)
            at += len(sel)
        want_sl = [(ref[b].primary[t] if prim else ref[b].secondary[t]) for b, t in targets]
        want_root = [ref[b].pair_hashes[t][0] if prim else ref[b].pair_hashes[n - 1 - t][1]
                     for b, t in targets]
        for (b, t), w in zip(targets, want_sl):  # the encoder's slivers too
            pair = enc[b][0][t if prim else n - 1 - t]
            assert (pair.primary if prim else pair.secondary).symbols.data == w.tobytes()
        erased = sum(any(i not in sel for i in range(K)) for sel in subs)
        v = SliverVerifier(n, s, axis)
        call = Call(n, s, axis, subs, datas, want_root)
        before = _stats()
        assert call.run(v) == OK, _lib.last_error()
        out, roots, verdict = call.results()
        for i in range(len(targets)):
            assert np.array_equal(out[i], want_sl[i]), (axis, i)
            assert roots[i].tobytes() == want_root[i]
        assert verdict.tolist() == [MATCH] * len(targets)
        call.assert_guards()
        assert (_stats() - before).tolist() == [1, erased, len(targets) - erased]
        # host form: a duplicate, an index >= n and a surplus symbol in every list
        idx, ptrs, keep, counts = [], [], [], []
        for sel, d in zip(subs, datas):
            rows = [(sel[0], d[0]), (n + 3, d[0])] + list(zip(sel, d)) + [(sel[1], d[1])]
            for i, a in rows:
                a = np.ascontiguousarray(a)
                keep.append(a)
                idx.append(i)
                ptrs.append(a.ctypes.data)
            counts.append(len(rows))
        m, tot = len(targets), len(idx)
        outs = [np.full(K * s + 8, FILL, dtype=np.uint8) for _ in range(m)]
        roots_h = np.zeros(m * 32, dtype=np.uint8)
        verdict_h = np.full(m, -1, dtype=np.int32)
        exp = np.frombuffer(b"".join(want_root), dtype=np.uint8)
        before = _stats()
        rc = _lib.lib().rs2_recover_slivers(
            n, s, 0 if prim else 1, m, (ctypes.c_uint32 * m)(*counts),
            (ctypes.c_uint16 * tot)(*idx), (ctypes.c_void_p * tot)(*ptrs), exp.ctypes.data,
            (ctypes.c_void_p * m)(*[o.ctypes.data for o in outs]), roots_h.ctypes.data,
            verdict_h.ctypes.data, None)
        assert rc == OK, _lib.last_error()
        for i in range(m):
            assert np.array_equal(outs[i][:K * s], want_sl[i]), (axis, i)
            assert (outs[i][K * s:] == FILL).all()
        assert roots_h.tobytes() == b"".join(want_root)
        assert verdict_h.tolist() == [MATCH] * m
        assert (_stats() - before).tolist() == [1, erased, m - erased]


# ---- 2. mismatch and corruption ---------------------------------------------------------------
@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_mismatch_and_corruption(gpu, axis):
    from walrus_amd.encoding import SliverVerifier
    n, s = 13, 22
    rng = np.random.default_rng(77)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(6)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]] for _ in slivers]
    v = SliverVerifier(n, s, axis)
    # one expected root zeroed
    call = _call_for(n, s, axis, slivers, subs)
    call.expected = b"".join(b"\0" * 32 if i == 2 else sl.root for i, sl in enumerate(slivers))
    assert call.run(v) == OK
    out, roots, verdict = call.results()
    assert verdict.tolist() == [MATCH, MATCH, MISMATCH, MATCH, MATCH, MATCH]
    for i, sl in enumerate(slivers):
        assert np.array_equal(out[i], sl.data.reshape(-1)) and roots[i].tobytes() == sl.root
    call.assert_guards()
    # one received repair symbol of sliver 3 with one byte flipped
    datas = [sl.all[sel].copy() for sl, sel in zip(slivers, subs)]
    j = next(j for j, q in enumerate(subs[3]) if q >= K)
    datas[3][j, 5] ^= 0x40
    call = Call(n, s, axis, subs, datas, [sl.root for sl in slivers])
    assert call.run(v) == OK
    out, roots, verdict = call.results()
    assert verdict.tolist() == [MATCH, MATCH, MATCH, MISMATCH, MATCH, MATCH]
    want = O.rs_decode_symbols(K, n, s, list(zip(subs[3], datas[3]))).reshape(-1)
    assert np.array_equal(out[3], want) and not np.array_equal(want, slivers[3].data.reshape(-1))
    assert roots[3].tobytes() == O.merkle_root(
        [x.tobytes() for x in O.rs_encode_all(want.reshape(K, s), n)])
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(out[i], slivers[i].data.reshape(-1))
        assert roots[i].tobytes() == slivers[i].root
    call.assert_guards()


# ---- 3. lane classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", [6, 22, 66, 130])
@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_lane_classes(gpu, axis, s):
    from walrus_amd.encoding import SliverVerifier
    n = 13
    rng = np.random.default_rng(s)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(5)]
    subs = _subsets(n, K, 5, rng)
    call = _call_for(n, s, axis, slivers, subs)
    assert call.run(SliverVerifier(n, s, axis)) == OK
    _check_exact(call, slivers)


# ---- 4. the C3 shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_c3_shape_one_launch(gpu, axis):
    from walrus_amd.encoding import SliverVerifier
    n, s, m = 1000, 20, 12
    rng = np.random.default_rng(1000)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(m)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]] for _ in slivers]
    call = _call_for(n, s, axis, slivers, subs)
    before = _stats()
    assert call.run(SliverVerifier(n, s, axis)) == OK
    _check_exact(call, slivers)
    assert (_stats() - before).tolist() == [1, m, 0]


# ---- 5. fallbacks: 2-byte symbols, more than 8 blocks ------------------------------------------
def test_fallback_two_byte_symbols(gpu):
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 10, 2, "primary"
    rng = np.random.default_rng(2)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(5)]
    subs = _subsets(n, K, 5, rng)
    call = _call_for(n, s, axis, slivers, subs)
    before = _stats()
    assert call.run(SliverVerifier(n, s, axis)) == OK
    _check_exact(call, slivers)
    assert (_stats() - before).tolist() == [0, 0, 5]


def test_fallback_more_than_eight_blocks_mixed(gpu):
    """n = 4500, s = 4: a random subset spans 16 transform blocks (per-sliver path), a one-erasure
    list stays within the batch job's 8 -- both in one call."""
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 4500, 4, "primary"
    rng = np.random.default_rng(4500)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(3)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]],
            [i for i in range(K) if i != 17] + [K + 5],
            [int(i) + 1 for i in rng.permutation(n - 1)[:K]]]
    call = _call_for(n, s, axis, slivers, subs)
    before = _stats()
    assert call.run(SliverVerifier(n, s, axis)) == OK
    _check_exact(call, slivers)
    d = (_stats() - before).tolist()
    assert d[2] >= 2 and d[1] + d[2] == 3, d


# ---- 6. more than one chunk, with gaps ---------------------------------------------------------
def test_more_than_one_chunk(gpu):
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 10, 6, "secondary"
    m = 2 * CHUNK_JOBS + 20
    rng = np.random.default_rng(6)
    K = _k(n, axis)
    base = [Sliver(n, K, s, rng) for _ in range(16)]
    slivers = [base[i % 16] for i in range(m)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]] for _ in range(m)]
    skipped = (5, CHUNK_JOBS - 1, CHUNK_JOBS, m - 1)
    for i in skipped:
        subs[i] = subs[i][:-1]
    subs[9] = list(range(K))  # a plain copy in the middle of a run
    call = _call_for(n, s, axis, slivers, subs)
    before = _stats()
    codes = call.run(SliverVerifier(n, s, axis), statuses=True)
    assert [i for i, c in enumerate(codes) if c != OK] == list(skipped)
    _check_exact(call, slivers, skipped)
    assert (_stats() - before).tolist() == [3, m - len(skipped) - 1, 1]


# ---- 7. back-to-back calls on one verifier -----------------------------------------------------
def test_back_to_back_calls(gpu):
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 13, 40, "primary"
    rng = np.random.default_rng(8)
    K = _k(n, axis)
    v = SliverVerifier(n, s, axis)
    calls = []
    for _ in range(3):  # three: the first chunk slot is taken again without a sync
        slivers = [Sliver(n, K, s, rng) for _ in range(7)]
        call = _call_for(n, s, axis, slivers, _subsets(n, K, 7, rng))
        assert call.run(v) == OK
        calls.append((call, slivers))
    for call, slivers in calls:
        _check_exact(call, slivers)


def test_verifier_stage_profiler(gpu):
    """rs2_verifier_profile_*: one span per stage of a profiled call, none once switched off."""
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 13, 22, "primary"
    rng = np.random.default_rng(14)
    K = _k(n, axis)
    v = SliverVerifier(n, s, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(4)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]] for _ in slivers]
    v.profile(True)
    call = _call_for(n, s, axis, slivers, subs)
    assert call.run(v) == OK
    _check_exact(call, slivers)
    stages = v.profile_read()
    assert set(stages) == {"rec_plan_host", "dec_batch_setup", "dec_batch_codec", "rec_roots",
                           "rec_verdict"}
    assert all(ms >= 0 and launches == 1 for ms, launches in stages.values()), stages
    v.profile(False)
    call = _call_for(n, s, axis, slivers, subs)
    assert call.run(v) == OK
    _check_exact(call, slivers)
    assert v.profile_read() == {}


# ---- 8. errors ---------------------------------------------------------------------------------
def test_errors_with_and_without_status(gpu):
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 10, 20, "primary"
    rng = np.random.default_rng(9)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(5)]
    subs = [[int(i) + 1 for i in rng.permutation(n - 1)[:K]] for _ in range(5)]
    subs[1] = subs[1][:-1]                      # one symbol short
    subs[3] = subs[3][:-1] + [subs[3][0]]       # K entries, K - 1 distinct
    good = subs[4]
    subs[4] = [good[0], n + 2] + good[1:] + [0]  # an index >= n among a surplus
    datas = [np.stack([sl.all[q] if q < n else np.zeros(s, dtype=np.uint8) for q in sel])
             for sl, sel in zip(slivers, subs)]
    v = SliverVerifier(n, s, axis)
    call = Call(n, s, axis, subs, datas, [sl.root for sl in slivers])
    before = _stats()
    codes = call.run(v, statuses=True)
    assert codes == [OK, E_UNSUCCESSFUL, OK, E_NOT_ENOUGH, OK]
    _check_exact(call, slivers, skipped=(1, 3))
    assert (_stats() - before).tolist() == [1, 3, 0]
    # status_out NULL: the first code, nothing written, no stats
    call = Call(n, s, axis, subs, datas, [sl.root for sl in slivers])
    before = _stats()
    assert call.run(v) == E_UNSUCCESSFUL
    torch.cuda.synchronize()
    call.assert_guards()
    for g in (call.out, call.roots, call.verdict):
        assert not g.changed([]), "a refused call wrote an output"
    assert (_stats() - before).tolist() == [0, 0, 0]
    # n_slivers = 0
    assert v.recover_slivers_async([], 0, 0) == OK
    # misaligned buffers
    ok_subs, ok_datas = [subs[0]], [datas[0]]
    c = Call(n, s, axis, ok_subs, ok_datas, [slivers[0].root])
    st = torch.cuda.current_stream().cuda_stream
    exp = c.expected
    assert v.recover_slivers_async(ok_subs, c.sym.ptr + 1, c.out.ptr, exp, c.roots.ptr,
                                   c.verdict.ptr, st) == E_INVALID
    assert v.recover_slivers_async(ok_subs, c.sym.ptr, c.out.ptr, exp, c.roots.ptr + 8,
                                   c.verdict.ptr, st) == E_INVALID
    assert v.recover_slivers_async(ok_subs, c.sym.ptr, c.out.ptr, exp, c.roots.ptr,
                                   c.verdict.ptr + 4, st) == E_INVALID
    # expected roots and verdicts go together
    assert v.recover_slivers_async(ok_subs, c.sym.ptr, c.out.ptr, None, c.roots.ptr,
                                   c.verdict.ptr, st) == E_INVALID
    torch.cuda.synchronize()
    c.assert_guards()
    assert not c.out.changed([]) and not c.roots.changed([]) and not c.verdict.changed([])
    # no expected roots: slivers and roots only
    c = Call(n, s, axis, ok_subs, ok_datas, None, verdict=False)
    assert c.run(v) == OK
    _check_exact(c, slivers[:1])


# ---- 9. containment -----------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0, 2, 6, 14])
def test_containment(gpu, delta):
    from walrus_amd.encoding import SliverVerifier
    n, s, axis = 13, 22, "secondary"
    rng = np.random.default_rng(10)
    K = _k(n, axis)
    slivers = [Sliver(n, K, s, rng) for _ in range(6)]
    subs = _subsets(n, K, 6, rng)
    subs[4] = subs[4][:-1]  # a skipped sliver between recovered ones
    v = SliverVerifier(n, s, axis)
    got = []
    for in_fill in (FILL, 99):
        call = _call_for(n, s, axis, slivers, subs, delta=delta, in_fill=in_fill)
        assert call.run(v, statuses=True)[4] == E_UNSUCCESSFUL
        _check_exact(call, slivers, skipped=(4,))
        got.append([a.copy() for a in call.results()])
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ---- 10. proof checks -----------------------------------------------------------------------------
def _proof_case(n, s, rng):
    """8 slivers' received symbols: sliver i has counts[i] symbols, all leaf targets[i] of their
    own source column (a random sliver's expansion), with proofs and roots from the oracle."""
    counts = [1, 65, 7, 130, 3, 64, 20, 5]
    K = _k(n, "primary")
    cols = [Sliver(n, K, s, rng) for _ in range(8)]  # source slivers, reused across requests
    leaves = [[x.tobytes() for x in c.all] for c in cols]
    targets = [int(t) for t in rng.integers(0, n - 1, 8)]
    targets[0] = n - 2
    syms, paths, roots = [], [], []
    memo = {}
    for cnt, t in zip(counts, targets):
        for j in range(cnt):
            c = j % 8
            if (c, t) not in memo:
                memo[(c, t)] = b"".join(O.merkle_proof(leaves[c], t))
            syms.append(cols[c].all[t].copy())
            paths.append(np.frombuffer(memo[(c, t)], dtype=np.uint8).copy())
            roots.append(np.frombuffer(cols[c].root, dtype=np.uint8).copy())
    return counts, targets, np.stack(syms), np.stack(paths), np.stack(roots)


def _host_flags(counts, targets, syms, paths, roots):
    """The proof step restated with hashlib (leaf 0x00 || data, inner 0x01 || left || right)."""
    def h(prefix, data):
        return hashlib.blake2b(prefix + data, digest_size=32).digest()
    flags, j = [], 0
    for cnt, t in zip(counts, targets):
        for _ in range(cnt):
            cur, idx = h(b"\0", syms[j].tobytes()), t
            p = paths[j].tobytes()
            for l in range(len(p) // 32):
                sib = p[32 * l:32 * l + 32]
                cur = h(b"\1", cur + sib) if idx % 2 == 0 else h(b"\1", sib + cur)
                idx //= 2
            flags.append(int(cur == roots[j].tobytes()))
            j += 1
    return flags


@pytest.mark.parametrize("n", [10, 1000])
def test_proof_checks(gpu, n):
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverVerifier
    s = 20
    rng = np.random.default_rng(n + 1)
    counts, targets, syms, paths, roots = _proof_case(n, s, rng)
    total = sum(counts)
    firsts = np.concatenate([[0], np.cumsum(counts)])
    assert O.merkle_proof_root([paths[0][i:i + 32].tobytes() for i in range(0, paths.shape[1], 32)],
                               syms[0].tobytes(), targets[0]) == roots[0].tobytes()
    v = SliverVerifier(n, s, "primary")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream

    def run(counts, targets, syms, paths, roots, delta=0, in_fill=FILL):
        g_sym = Guarded(syms.size, delta, dev, fill=in_fill).set(syms)
        g_path = Guarded(paths.size, 0, dev, fill=in_fill).set(paths)
        g_root = Guarded(roots.size, 0, dev, fill=in_fill).set(roots)
        g_ok = Guarded(total, 0, dev, fill=FILL)
        rc = v.check_recovery_symbols_async(counts, targets, g_sym.ptr, g_path.ptr, g_root.ptr,
                                            g_ok.ptr, st)
        assert rc == OK, _lib.last_error()
        torch.cuda.synchronize()
        for g, a in ((g_sym, syms), (g_path, paths), (g_root, roots)):
            g.assert_guards_intact(what="an input")
            assert np.array_equal(g.numpy(), a.reshape(-1)), "an input was written"
        g_ok.assert_guards_intact(what="d_ok")
        flags = g_ok.numpy().tolist()
        assert flags == _host_flags(counts, targets, syms, paths, roots)
        return flags

    for delta in (0, 2, 6, 14):
        assert run(counts, targets, syms, paths, roots, delta, 50 + delta) == [1] * total
    j = int(firsts[3]) + 70  # a symbol of the second workgroup of sliver 3
    one = [int(i != j) for i in range(total)]
    bad = syms.copy()
    bad[j, 3] ^= 1
    assert run(counts, targets, bad, paths, roots) == one
    bad = paths.copy()
    bad[j, 32 * (paths.shape[1] // 32 - 1) + 9] ^= 0x80  # the last path node
    assert run(counts, targets, syms, bad, roots) == one
    bad = roots.copy()
    bad[j, 31] ^= 2
    assert run(counts, targets, syms, paths, bad) == one
    moved = list(targets)
    moved[3] += 1
    want = [int(not (firsts[3] <= i < firsts[4])) for i in range(total)]
    assert run(counts, moved, syms, paths, roots) == want
    # the host form, and a target index >= n
    ok = np.full(total, 9, dtype=np.uint8)
    m = len(counts)
    rc = _lib.lib().rs2_check_recovery_symbols(
        n, s, 0, m, (ctypes.c_uint32 * m)(*counts), (ctypes.c_uint16 * m)(*targets),
        syms.ctypes.data, paths.ctypes.data, roots.ctypes.data, ok.ctypes.data)
    assert rc == OK and ok.tolist() == [1] * total
    g_ok = Guarded(total, 0, dev, fill=FILL)
    d = [torch.from_numpy(a).to(dev) for a in (syms, paths, roots)]
    assert v.check_recovery_symbols_async(counts, targets[:-1] + [n], d[0].data_ptr(),
                                          d[1].data_ptr(), d[2].data_ptr(), g_ok.ptr,
                                          st) == E_INVALID
    assert v.check_recovery_symbols_async(counts, targets, d[0].data_ptr(), d[1].data_ptr() + 8,
                                          d[2].data_ptr(), g_ok.ptr, st) == E_INVALID
    torch.cuda.synchronize()
    assert not g_ok.changed([])


# ---- 11. the Python layer --------------------------------------------------------------------------
def test_python_layer_matches_single_sliver_functions(gpu):
    R = gpu.recovery
    n = 10
    cfg = gpu.ReedSolomonEncodingConfig(n)
    rng = np.random.default_rng(12)
    blobs = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (314, 300)]
    enc = [cfg.encode_with_metadata(b) for b in blobs]
    for axis, orth in ((gpu.PRIMARY, gpu.SECONDARY), (gpu.SECONDARY, gpu.PRIMARY)):
        need = cfg.n_symbols_for_recovery(axis)
        requests = []
        for b, (pairs, meta) in enumerate(enc):
            for pair_t in (0, 4):
                chosen = [int(i) for i in rng.permutation(n) if int(i) != pair_t][:need + 1]
                src = [pairs[i].secondary if axis == gpu.PRIMARY else pairs[i].primary
                       for i in chosen]
                syms = gpu.recovery_symbols_for_requests(cfg, src, [pair_t] * len(src))
                target = pair_t if axis == gpu.PRIMARY else n - 1 - pair_t
                requests.append((syms, target, meta.metadata))
        md0 = requests[0][2]
        pair0 = requests[0][1] if axis == gpu.PRIMARY else n - 1 - requests[0][1]
        bad = gpu.BlobMetadata(
            [((b"\0" * 32, h[1]) if axis == gpu.PRIMARY else (h[0], b"\0" * 32))
             if i == pair0 else h for i, h in enumerate(md0.hashes)], md0.unencoded_length)
        requests.append((requests[0][0], requests[0][1], bad))
        requests.append((requests[1][0][:need - 1], requests[1][1], requests[1][2]))
        flags = gpu.verify_recovery_symbols(cfg, [r[2] for r in requests],
                                            [r[1] for r in requests],
                                            [r[0] for r in requests], axis)
        for (syms, target, meta), fl in zip(requests, flags):
            want = []
            for r in syms:
                try:
                    r.verify(n, cfg.symbol_size_for_blob(meta.unencoded_length), meta, target)
                    want.append(True)
                except R.SymbolVerificationError:
                    want.append(False)
            assert fl == want and all(fl)
        tampered = list(requests[2][0])
        t0 = tampered[1]
        tampered[1] = R.RecoverySymbol(t0.axis, t0.index, bytes([t0.data[0] ^ 1]) + t0.data[1:],
                                       t0.proof)
        fl = gpu.verify_recovery_symbols(cfg, [requests[2][2]], [requests[2][1]], [tampered],
                                         axis)[0]
        assert fl == [i != 1 for i in range(len(tampered))]
        got = gpu.recover_slivers_or_generate_inconsistency_proofs(cfg, requests, axis)
        assert len(got) == len(requests)
        for (syms, target, meta), g in zip(requests, got):
            try:
                want = gpu.recover_sliver_or_generate_inconsistency_proof(syms, target, meta, cfg,
                                                                          axis)
            except R.SliverRecoveryError:
                assert isinstance(g, R.SliverRecoveryError)
                continue
            assert type(g) is type(want)
            if isinstance(want, gpu.SliverData):
                assert (g.symbols.data, g.index, g.axis) == (want.symbols.data, want.index,
                                                             want.axis)
            else:
                assert (g.axis, g.target_sliver_index) == (want.axis, want.target_sliver_index)
                assert [r.index for r in g.recovery_symbols] == \
                    [r.index for r in want.recovery_symbols]
        assert isinstance(got[-2], gpu.InconsistencyProof)
        got[-2].verify(bad, cfg)
        assert isinstance(got[-1], R.SliverRecoveryError)
        assert all(isinstance(g, gpu.SliverData) for g in got[:-2])
