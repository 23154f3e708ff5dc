"""The paths of rs2_decode_and_verify_batch_device_async that one model call does not take: more
than one window (by blob count and by the byte budget), the counters, refused blobs with and
without status_out, the argument rules, and agreement with rs2_decode_and_verify_device on a
call that mixes batched and per-blob decodes."""
import numpy as np
import pytest

import corruption as C
import rs2_oracle as O
import verify_batch as VB

pytestmark = pytest.mark.gpu

OK, E_NOT_ENOUGH, E_UNSUCCESSFUL, E_INVALID = 0, -5, -6, -8
SKIP, DEFAULT, STRICT = 0, 1, 2


def _stats():
    from walrus_amd.encoding import verify_batch_stats
    return verify_batch_stats()


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _rows_of(cases):
    """Per case, the number of rows the model's Default check hashes."""
    out = []
    for c in cases:
        g = C.GEOMETRIES[c.geo]
        axis, idx = C.layouts(c.geo)[c.layout]
        p = O.Rs2Params.for_blob(g.n, g.length)
        out.append(len(VB.model_rows(p, axis, idx, g.length + c.dlen)))
    return out


@pytest.mark.parametrize("check", ["default", "strict"])
def test_two_blob_count_windows(gpu, check):
    """G1's primary cases three times over: 372 blobs, two windows of at most 341."""
    g = C.GEOMETRIES["G1"]
    cases = VB.batch_cases("G1", C.PRIMARY, check, honest_every=10 ** 9) * 3
    assert len(cases) == 372
    want = VB.model_verdicts(cases)
    plan = gpu.DevicePlan(g.n, g.length)
    packed = VB.pack(cases)
    call = VB.DeviceCall(gpu, plan, packed)
    before = _stats()
    verdicts, out, _ = call.run(packed, check)
    d = _delta(_stats(), before)
    VB.assert_against_model(cases, want, verdicts, out, packed.lens)
    assert d["windows"] == 2 and d["checked"] == 372
    if check == "default":
        assert d["rows"] == sum(_rows_of(cases)) and d["encoded"] == 0
    else:
        assert d["encoded"] == 372 and d["rows"] == 0


@pytest.mark.parametrize("check", ["default", "strict"])
def test_byte_budget(gpu, check):
    """G4 with the budget at one blob's need: the verdicts do not change, every blob that needs
    scratch gets a window of its own."""
    g = C.GEOMETRIES["G4"]
    p = O.Rs2Params.for_blob(g.n, g.length)
    cases = VB.batch_cases("G4", C.PRIMARY, check)
    want = VB.model_verdicts(cases)
    plan = gpu.DevicePlan(g.n, g.length)
    packed = VB.pack(cases)
    call = VB.DeviceCall(gpu, plan, packed)
    if check == "strict":
        need = [VB.strict_need(p)] * len(cases)
    else:
        need = [VB.default_need(p, r) for r in _rows_of(cases)]
    budget = max(need)
    assert VB.windows(need, 256 << 20) == 1
    try:
        gpu.set_verify_batch_budget(budget)
        before = _stats()
        verdicts, out, _ = call.run(packed, check)
        d = _delta(_stats(), before)
    finally:
        gpu.set_verify_batch_budget(0)
    VB.assert_against_model(cases, want, verdicts, out, packed.lens)
    assert d["windows"] == VB.windows(need, budget)
    if check == "strict":
        assert d["windows"] == len(cases)
    else:
        assert d["windows"] > len(cases) // 2 and d["rows"] == sum(_rows_of(cases))
    # the default is back: one window again
    before = _stats()
    verdicts2, _, _ = call.run(packed, check)
    assert _delta(_stats(), before)["windows"] == 1 and (verdicts2 == verdicts).all()


def _with_invalid(packed, g, p):
    """Every fifth blob invalid, three kinds in turn: (blobs, lens, codes)."""
    blobs, lens = [(list(ix), list(of)) for ix, of in packed.blobs], list(packed.lens)
    codes = [OK] * len(blobs)
    need = p.n_primary if packed.axis == C.PRIMARY else p.n_secondary
    for k, b in enumerate(range(2, len(blobs), 5)):
        ix, of = blobs[b]
        if k % 3 == 0:       # one sliver short
            cut = need - 1
            while len(set(ix[:cut + 1])) < need:
                cut += 1
            blobs[b], codes[b] = (ix[:cut], of[:cut]), E_UNSUCCESSFUL
            assert len(set(ix[:cut])) == need - 1
        elif k % 3 == 1:     # an index >= n
            blobs[b], codes[b] = ([g.n] + ix[1:], of), E_NOT_ENOUGH
        else:                # a length of another symbol size
            lens[b] = p.n_primary * p.n_secondary * g.symbol_size + 1
            codes[b] = E_INVALID
    return blobs, lens, codes


@pytest.mark.parametrize("check", ["default", "strict"])
@pytest.mark.parametrize("axis", [C.PRIMARY, C.SECONDARY])
def test_status_out_and_refused_blobs(gpu, axis, check):
    g = C.GEOMETRIES["G3"]
    p = O.Rs2Params.for_blob(g.n, g.length)
    cases = VB.batch_cases("G3", axis, check)[:60]
    want = VB.model_verdicts(cases)
    plan = gpu.DevicePlan(g.n, g.length)
    packed = VB.pack(cases)
    stride = p.n_primary * p.n_secondary * g.symbol_size + 40   # holds the overlong length too
    call = VB.DeviceCall(gpu, plan, packed, out_stride=stride)
    blobs, lens, codes = _with_invalid(packed, g, p)
    assert {E_UNSUCCESSFUL, E_NOT_ENOUGH, E_INVALID} <= set(codes)
    before = _stats()
    verdicts, out, st = call.run(packed, check, statuses=True, blobs=blobs, lens=lens)
    d = _delta(_stats(), before)
    assert st == codes
    good = [b for b, c in enumerate(codes) if c == OK]
    for b, c in enumerate(codes):
        if c != OK:
            assert verdicts[b] == VB.SKIPPED, b
            assert (out[b] == VB.OUT_FILL).all(), f"refused blob {b}: its slot was written"
    VB.assert_against_model([cases[b] for b in good], [want[b] for b in good], verdicts[good],
                            out[good], [lens[b] for b in good])
    assert d["checked"] == len(good)

    # status_out NULL: the first code, outputs and verdicts untouched
    import torch
    call.out.fill_(VB.OUT_FILL)
    call.verdict.fill_(VB.VERDICT_FILL)
    torch.cuda.synchronize()
    before = _stats()
    rc, _ = VB.raw_call(plan, axis, blobs, lens, call.slivers.data_ptr(), call.hashes.data_ptr(),
                        call.ids.data_ptr(), DEFAULT if check == "default" else STRICT,
                        call.out.data_ptr(), stride, call.verdict.data_ptr())
    plan.sync()
    torch.cuda.synchronize()
    assert rc == next(c for c in codes if c != OK)
    assert _delta(_stats(), before)["windows"] == 0
    assert bool((call.out == VB.OUT_FILL).all())
    assert bool((call.verdict == VB.VERDICT_FILL).all())


def test_argument_rules(gpu):
    import torch
    g = C.GEOMETRIES["G1"]
    cases = VB.batch_cases("G1", C.PRIMARY, "default")[:8]
    plan = gpu.DevicePlan(g.n, g.length)
    packed = VB.pack(cases)
    call = VB.DeviceCall(gpu, plan, packed)
    call.slivers.copy_(torch.from_numpy(packed.slivers))
    call.hashes.copy_(torch.from_numpy(packed.hashes))
    call.ids.copy_(torch.from_numpy(packed.ids))
    torch.cuda.synchronize()
    sl, h, i, o, v = (t.data_ptr() for t in (call.slivers, call.hashes, call.ids, call.out,
                                             call.verdict))
    assert h % 16 == 0 and i % 16 == 0 and v % 16 == 0

    def rc(check, d_hashes=h, d_ids=i, d_verdict=v, n_blobs=None):
        code, _ = VB.raw_call(plan, C.PRIMARY, packed.blobs, packed.lens, sl, d_hashes, d_ids,
                              check, o, call.out_stride, d_verdict, n_blobs=n_blobs)
        plan.sync()
        return code

    before = _stats()
    assert rc(DEFAULT, n_blobs=0) == OK
    assert rc(DEFAULT, d_hashes=0) == E_INVALID
    assert rc(STRICT, d_ids=0) == E_INVALID
    assert rc(3) == E_INVALID and rc(-1) == E_INVALID
    assert rc(DEFAULT, d_hashes=h + 8) == E_INVALID
    assert rc(STRICT, d_ids=i + 8) == E_INVALID
    assert rc(DEFAULT, d_verdict=v + 4) == E_INVALID
    assert rc(DEFAULT, d_verdict=0) == E_INVALID
    assert _delta(_stats(), before)["windows"] == 0   # nothing of the above enqueued a window
    # the pointer the check does not read may be NULL
    want = {chk: [VB.MATCH if w[0] == "ok" else VB.MISMATCH for w in VB.model_verdicts(
        [C.replace(c, check=chk) for c in cases])] for chk in C.CHECKS}
    for check, name, kw in ((STRICT, "strict", dict(d_hashes=0)), (DEFAULT, "default", dict(d_ids=0)),
                            (SKIP, "skip", dict(d_hashes=0, d_ids=0))):
        call.verdict.fill_(VB.VERDICT_FILL)
        torch.cuda.synchronize()
        assert rc(check, **kw) == OK
        torch.cuda.synchronize()
        assert call.verdict.cpu().tolist() == want[name], name


def test_agrees_with_the_single_blob_call(gpu):
    """(34, 100) at block limit 8: 90 patterns run as batched jobs, one takes the per-blob
    decode.  One byte is flipped in a used sliver of every third blob; each blob's verdict equals
    what rs2_decode_and_verify_device says about the same slivers alone."""
    import torch
    from erasure_patterns import batch_jobs, block_limit, families
    from walrus_amd.encoding import decode_batch_stats
    k, n, limit = 34, 100, 8
    length = 34 * 67 * 6 - 201
    p = O.Rs2Params.for_blob(n, length)
    assert (p.n_primary, p.symbol_size) == (k, 6)
    blob = np.random.default_rng(5).integers(0, 256, length, dtype=np.uint8).tobytes()
    prim, _, hashes, bid = C.backend(n).encode(blob, n)
    jobs = batch_jobs(families(k, n, limit))
    ln = prim.shape[1]
    parts, blobs = [], []
    for j, (_, sel, _) in enumerate(jobs):
        sl = prim[list(sel)].copy()
        if j % 3 == 0:
            sl[j % k, (7 * j) % ln] ^= 0x10
        blobs.append((list(sel), [(j * k + q) * ln for q in range(k)]))
        parts.append(sl.reshape(-1))
    B = len(jobs)
    dev = torch.device("cuda", 0)
    d_sl = torch.from_numpy(np.concatenate(parts)).to(dev)
    hb = b"".join(a + b for a, b in hashes)
    d_h = torch.from_numpy(np.frombuffer(hb * B, np.uint8).copy()).to(dev)
    d_i = torch.from_numpy(np.frombuffer(bid * B, np.uint8).copy()).to(dev)
    stride = length + 39
    d_out = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
    d_v = torch.zeros(B, dtype=torch.int32, device=dev)
    d_one = torch.zeros(length + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with block_limit(limit):
        plan = gpu.DevicePlan(n, length)
        for check in ("default", "strict"):
            alone = []
            for ix, of in blobs:
                try:
                    plan.decode_and_verify(C.PRIMARY, ix, d_sl.data_ptr(), of, hb, bid, check,
                                           d_one.data_ptr())
                    alone.append(VB.MATCH)
                except gpu.VerificationError:
                    alone.append(VB.MISMATCH)
            d_v.fill_(VB.VERDICT_FILL)
            torch.cuda.synchronize()
            before = decode_batch_stats()
            plan.decode_and_verify_batch_async(C.PRIMARY, blobs, d_sl.data_ptr(), d_out.data_ptr(),
                                               stride, d_h.data_ptr(), d_i.data_ptr(), check,
                                               d_v.data_ptr())
            plan.sync()
            torch.cuda.synchronize()
            after = decode_batch_stats()
            assert d_v.cpu().tolist() == alone, check
            assert VB.MATCH in alone and VB.MISMATCH in alone
            assert after["batched"] - before["batched"] == 90
            assert after["single"] - before["single"] == 1
        del plan
