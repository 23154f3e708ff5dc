"""Verdicts, refusals, host forms and the Python layer of the mixed sliver recovery, and the
mixed proof check.

Verdicts: every 7th sliver gets its neighbour's expected root, every 11th one flipped bit in a
received symbol (a present original and a repair symbol in turn); MISMATCH appears exactly there,
the output equals the oracle's decode of what was received, every other sliver is exact.
Refusals: each per-sliver rule is reached in the stated order -- a sliver that breaks two rules
gets the code of the earlier one -- with status_out NULL (the first code, nothing written) and
non-NULL (skipped: output and root slot untouched, verdict SKIPPED; the rest run)."""
import ctypes

import numpy as np
import pytest
import torch

import erasure_patterns as EP
import recover_mixed as R
import rs2_oracle as O
import verify_mixed as M
from walrus_amd import _lib

pytestmark = pytest.mark.gpu

N = 13
INVALID, INCOMPATIBLE = _lib.RS2_E_INVALID_ARGUMENT, _lib.RS2_E_INCOMPATIBLE_PARAMETERS
UNSUCCESSFUL, NOT_ENOUGH = _lib.RS2_E_DECODING_UNSUCCESSFUL, _lib.RS2_E_NOT_ENOUGH_SHARDS


def test_mismatches_exactly_where_planted(gpu):
    items = R.family_case(N, R.SIZES)
    m = len(items)
    roots = R.expected_roots(N, items)
    expected = bytearray(roots)
    data, want, planted = [None] * m, [None] * m, set()
    for i in range(0, m, 7):
        j = (i + 1) % m
        if roots[32 * j:32 * j + 32] != roots[32 * i:32 * i + 32]:
            expected[32 * i:32 * i + 32] = roots[32 * j:32 * j + 32]
            planted.add(i)
    turn = 0
    for i in range(3, m, 11):
        a, s, pat, _ = items[i]
        k = R.k_of(N, a)
        pool = [p for p, q in enumerate(pat) if (q < k) == (turn % 2 == 0)] or list(range(len(pat)))
        turn += 1
        pos = pool[i % len(pool)]
        rec = R.received(N, items[i]).copy()
        rec[pos * s + (i % s)] ^= 1 << (i % 8)
        data[i] = rec.tobytes()
        dec = O.rs_decode_symbols(k, N, s, [(q, rec[p * s:(p + 1) * s]) for p, q in enumerate(pat)])
        want[i] = np.asarray(dec, dtype=np.uint8).reshape(-1).tobytes()
        assert want[i] != R.want_sliver(N, items[i])
        planted.add(i)
    rc, out, o_off, got_roots, verdict = R.run(gpu.SliverChecker(N), N, items,
                                               expected=bytes(expected), data=data)
    assert rc == 0, (rc, _lib.last_error())
    R.check_slivers(N, items, out, o_off, want=want, what="planted")
    assert verdict == [R.MISMATCH if i in planted else R.MATCH for i in range(m)]
    for i in range(m):
        if want[i] is None:
            assert got_roots[32 * i:32 * i + 32] == roots[32 * i:32 * i + 32], i
        else:
            a, s = items[i][:2]
            assert got_roots[32 * i:32 * i + 32] == M.root_of(N, s, a, want[i]), i


def _refusal_case():
    """[(what, code, item overrides)]: the sliver breaks the named rule and, where it can, every
    later one too, so the order of the checks decides its code."""
    kp, ks = R.k_of(N, "secondary"), R.k_of(N, "primary")
    short = list(range(ks - 1))
    dup = [0] * (ks + 1)
    return [
        ("axis", INVALID, dict(axis=2, s=5, sym_odd=True, idx=short)),
        ("size odd", INCOMPATIBLE, dict(s=5, sym_odd=True, idx=short)),
        ("size zero", INCOMPATIBLE, dict(s=0, out_odd=True, idx=short)),
        ("symbols_off odd", INVALID, dict(sym_odd=True, idx=short)),
        ("sliver_off odd", INVALID, dict(out_odd=True, idx=dup)),
        ("count below K", UNSUCCESSFUL, dict(idx=[0] * (ks - 1))),
        ("not enough distinct", NOT_ENOUGH, dict(idx=dup)),
        ("index past n", NOT_ENOUGH, dict(idx=list(range(ks - 1)) + [N, N + 5])),
    ], kp, ks


def _call(checker, items, bad_at, over, statuses):
    """The good `items` with sliver bad_at replaced by the overrides; returns (result, output
    numpy, output offsets, roots, verdicts)."""
    axes = [a for a, _, _, _ in items]
    sizes = [s for _, s, _, _ in items]
    idx = [list(p) for _, _, p, _ in items]
    s_off, s_size, o_off, o_size = R.layout(N, items)
    s_off, o_off = list(s_off), list(o_off)
    if bad_at is not None:
        axes[bad_at] = over.get("axis", axes[bad_at])
        sizes[bad_at] = over.get("s", sizes[bad_at])
        idx[bad_at] = over["idx"]
        s_off[bad_at] += 1 if over.get("sym_odd") else 0
        o_off[bad_at] += 1 if over.get("out_odd") else 0
    m = len(items)
    d_sym = torch.tensor(R.payload(N, items, R.layout(N, items)[0], s_size), dtype=torch.uint8,
                         device=R.dev())
    d_out = torch.full((o_size,), R.FILL, dtype=torch.uint8, device=R.dev())
    d_roots = torch.full((m * 32,), R.FILL, dtype=torch.uint8, device=R.dev())
    d_verdict = torch.full((m * 4,), R.FILL, dtype=torch.uint8, device=R.dev())
    torch.cuda.synchronize()
    res = checker.recover_async(axes, sizes, idx, d_sym.data_ptr(), s_off, d_out.data_ptr(), o_off,
                                R.expected_roots(N, items), d_roots.data_ptr(),
                                d_verdict.data_ptr(), None, statuses)
    torch.cuda.synchronize()
    return (res, d_out.cpu().numpy(), R.layout(N, items)[2], d_roots.cpu().numpy().tobytes(),
            d_verdict.cpu().numpy().view(np.int32).tolist())


def test_refusals_in_order(gpu):
    cases, kp, ks = _refusal_case()
    fams = EP.families(ks, N)
    items = [("primary", s, R.handed_over(fams[3 * j][1], j), j) for j, s in enumerate([6, 66, 130])]
    checker = gpu.SliverChecker(N)
    for what, code, over in cases:
        before = R.stats()
        res, out, o_off, roots, verdict = _call(checker, items, 1, over, statuses=False)
        assert res == code, (what, res, _lib.last_error())
        assert (out == R.FILL).all() and roots == bytes([R.FILL]) * 96, what
        assert verdict == [int.from_bytes(bytes([R.FILL]) * 4, "little", signed=True)] * 3, what
        assert R.moved(before) == [0] * 5, what
        res, out, o_off, roots, verdict = _call(checker, items, 1, over, statuses=True)
        assert res == [0, code, 0], (what, res)
        R.check_slivers(N, items, out, o_off, skipped={1}, what=what)
        R.check_roots(N, items, roots, skipped={1}, what=what)
        assert verdict == [R.MATCH, R.SKIPPED, R.MATCH], what


def _ptrs(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def test_host_form(gpu):
    n = 10
    items = R.family_case(n, [4, 66, 130, 258])[:20]
    m = len(items)
    ks = R.k_of(n, "primary")
    lists = [list(p) for _, _, p, _ in items]
    lists[2] = lists[2][:-1]                               # count below K
    lists[5] = [lists[5][0]] * len(lists[5])               # not enough distinct shards
    skipped = {2: UNSUCCESSFUL, 5: NOT_ENOUGH}
    axes = (ctypes.c_uint8 * m)(*[R.AXES.index(a) for a, _, _, _ in items])
    sizes = (ctypes.c_uint16 * m)(*[s for _, s, _, _ in items])
    counts = (ctypes.c_uint32 * m)(*[len(x) for x in lists])
    flat = [q for x in lists for q in x]
    idx = (ctypes.c_uint16 * len(flat))(*flat)
    keep = []
    for it, lst in zip(items, lists):
        cw = R.codeword(n, it[1], it[0], it[3])
        keep += [np.ascontiguousarray(cw[q]) for q in lst]
    expected = np.frombuffer(R.expected_roots(n, items), dtype=np.uint8).copy()
    expected[32 * 7:32 * 8] ^= 0xFF                        # one mismatch
    bufs = [np.full(R.k_of(n, a) * s, R.FILL, dtype=np.uint8) for a, s, _, _ in items]
    roots = np.full(m * 32, R.FILL, dtype=np.uint8)
    verdict = np.full(m, -1, dtype=np.int32)
    status = (ctypes.c_int * m)()
    fn = _lib.lib().rs2_recover_slivers_mixed
    rc = fn(n, m, axes, sizes, counts, idx, _ptrs(keep), expected.ctypes.data, _ptrs(bufs),
            roots.ctypes.data, verdict.ctypes.data, status)
    assert rc == 0, (rc, _lib.last_error())
    assert list(status) == [skipped.get(i, 0) for i in range(m)]
    want_roots = R.expected_roots(n, items)
    for i, it in enumerate(items):
        if i in skipped:
            assert (bufs[i] == R.FILL).all() and (roots[32 * i:32 * i + 32] == R.FILL).all()
            assert verdict[i] == R.SKIPPED
            continue
        assert bufs[i].tobytes() == R.want_sliver(n, it), i
        assert roots[32 * i:32 * i + 32].tobytes() == want_roots[32 * i:32 * i + 32], i
        assert verdict[i] == (R.MISMATCH if i == 7 else R.MATCH)
    # status_out NULL: the first failing sliver's code, nothing written
    bufs2 = [np.full(b.size, R.FILL, dtype=np.uint8) for b in bufs]
    rc = fn(n, m, axes, sizes, counts, idx, _ptrs(keep), None, _ptrs(bufs2), None, None, None)
    assert rc == UNSUCCESSFUL and all((b == R.FILL).all() for b in bufs2)


def test_python_layer_on_real_blobs(gpu):
    RC = gpu.recovery
    n = 10
    cfg = gpu.ReedSolomonEncodingConfig(n)
    rng = np.random.default_rng(20)
    enc = [cfg.encode_with_metadata(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
           for ln in (314, 3000, 41)]
    assert len({cfg.symbol_size_for_blob(m.metadata.unencoded_length) for _, m in enc}) == 3
    requests = []
    for axis in (gpu.PRIMARY, gpu.SECONDARY):
        need = cfg.n_symbols_for_recovery(axis)
        for pairs, meta in enc:
            for pair_t in (0, 4):
                chosen = [int(i) for i in rng.permutation(n) if int(i) != pair_t][:need + 1]
                src = [pairs[i].secondary if axis == gpu.PRIMARY else pairs[i].primary
                       for i in chosen]
                syms = gpu.recovery_symbols_for_requests(cfg, src, [pair_t] * len(src))
                target = pair_t if axis == gpu.PRIMARY else n - 1 - pair_t
                requests.append((syms, target, meta.metadata, axis))
    syms0, t0, md0, ax0 = requests[0]
    bad = gpu.BlobMetadata([((b"\0" * 32, h[1]) if i == t0 else h)
                            for i, h in enumerate(md0.hashes)], md0.unencoded_length)
    requests.append((syms0, t0, bad, ax0))
    need0 = cfg.n_symbols_for_recovery(requests[1][3])
    requests.append((requests[1][0][:need0 - 1],) + requests[1][1:])
    flags = gpu.verify_recovery_symbols_of_blobs(cfg, [(r[2], r[1], r[0], r[3]) for r in requests])
    for k, ((syms, target, meta, axis), fl) in enumerate(zip(requests, flags)):
        want = gpu.verify_recovery_symbols(cfg, [meta], [target], [syms], axis)[0]
        # (the altered metadata changes the target's own hash, not the source slivers' hashes the
        # symbols authenticate against)
        assert fl == want and all(fl), k
    tampered = list(requests[3][0])
    s1 = tampered[1]
    tampered[1] = RC.RecoverySymbol(s1.axis, s1.index, bytes([s1.data[0] ^ 1]) + s1.data[1:],
                                    s1.proof)
    fl = gpu.verify_recovery_symbols_of_blobs(
        cfg, [(requests[2][2], requests[2][1], requests[2][0], requests[2][3]),
              (requests[3][2], requests[3][1], tampered, requests[3][3])])
    assert all(fl[0]) and fl[1] == [i != 1 for i in range(len(tampered))]
    before = R.stats()
    got = gpu.recover_slivers_of_blobs(cfg, requests)
    assert R.moved(before)[0] == 1, "more than one mixed call's window"
    assert len(got) == len(requests)
    for (syms, target, meta, axis), g in zip(requests, got):
        try:
            want = gpu.recover_sliver_or_generate_inconsistency_proof(syms, target, meta, cfg, axis)
        except RC.SliverRecoveryError:
            assert isinstance(g, RC.SliverRecoveryError)
            continue
        assert type(g) is type(want)
        if isinstance(want, gpu.SliverData):
            assert (g.symbols.data, g.index, g.axis) == (want.symbols.data, want.index, want.axis)
        else:
            assert (g.axis, g.target_sliver_index) == (want.axis, want.target_sliver_index)
            assert [r.index for r in g.recovery_symbols] == [r.index for r in want.recovery_symbols]
    assert isinstance(got[-2], gpu.InconsistencyProof)
    got[-2].verify(bad, cfg)
    assert isinstance(got[-1], RC.SliverRecoveryError)
    assert all(isinstance(g, gpu.SliverData) for g in got[:-2])


@pytest.mark.parametrize("n", [13, 100])
def test_proof_check_against_the_oracle(gpu, n):
    """Sliver i's received symbols are symbol t_i of `count` source slivers' expansions, each with
    its O.merkle_proof path and root; one tampered path node and one tampered symbol per size."""
    sizes = [4, 6, 62, 66, 130, 254, 258]
    L = len(O.merkle_proof([b"\0\0"] * n, 0))
    counts, targets, runs, proofs, roots, want = [], [], [], [], [], []
    for g, s in enumerate(sizes):
        a = R.AXES[g % 2]
        count, t = 3 + g % 3, (5 * g + 1) % n
        run = bytearray()
        for j in range(count):
            leaves = [bytes(x) for x in R.codeword(n, s, a, j)]
            sym, path = bytearray(leaves[t]), [bytearray(x) for x in O.merkle_proof(leaves, t)]
            ok = True
            if j == 0 and L:
                path[g % L][g % 32] ^= 0x10
                ok = False
            if j == 1:
                sym[(3 * g) % s] ^= 0x01
                ok = False
            run += sym
            proofs.append(b"".join(bytes(x) for x in path))
            roots.append(O.merkle_root(leaves))
            want.append(int(ok))
        counts.append(count)
        targets.append(t)
        runs.append(bytes(run))
    off, at = [], 0
    for r in runs:
        off.append(at)
        at += len(r) + 2
    buf = np.full(at, 0x5A, dtype=np.uint8)
    for o, r in zip(off, runs):
        buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    total = sum(counts)
    d_sym = torch.tensor(buf, device=R.dev())
    d_proofs = torch.tensor(np.frombuffer(b"".join(proofs) or b"\0" * 32, dtype=np.uint8).copy(),
                            device=R.dev())
    d_roots = torch.tensor(np.frombuffer(b"".join(roots), dtype=np.uint8).copy(), device=R.dev())
    d_ok = torch.full((total,), R.FILL, dtype=torch.uint8, device=R.dev())
    torch.cuda.synchronize()
    rc = gpu.SliverChecker(n).check_recovery_symbols_async(
        sizes, counts, targets, d_sym.data_ptr(), off, d_proofs.data_ptr(), d_roots.data_ptr(),
        d_ok.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.last_error())
    assert d_ok.cpu().tolist() == want
    # the host form over the same symbols
    keep = [np.frombuffer(r, dtype=np.uint8)[j * s:(j + 1) * s].copy()
            for r, s, c in zip(runs, sizes, counts) for j in range(c)]
    ok = np.full(total, R.FILL, dtype=np.uint8)
    rc = _lib.lib().rs2_check_recovery_symbols_mixed(
        n, len(sizes), (ctypes.c_uint16 * len(sizes))(*sizes),
        (ctypes.c_uint32 * len(sizes))(*counts), (ctypes.c_uint16 * len(sizes))(*targets),
        _ptrs(keep), b"".join(proofs), b"".join(roots), ok.ctypes.data)
    assert rc == 0, (rc, _lib.last_error())
    assert ok.tolist() == want
