"""Batched blob decode (DevicePlan.decode_batch_async) under the structured erasure patterns.

One call carries EVERY family pattern of a geometry (erasure_patterns.BATCH_CALLS), a
pattern per job, so one launch holds what tests/test_erasure_patterns.py proves on the CPU: jobs
of 1 to 8 input and 1 to 5 output blocks side by side (the launch is as deep as the deepest job;
a workgroup past its own job's n_out leaves), mixing rows of n_in < 8 beside n_in == 8, jobs with
and without the P/Q block pair, with and without the fused copy of present originals, and jobs of
more than 8 blocks that take the per-blob decode between batched ones.  Job j decodes blob
j % 4 of four blobs of one symbol size and different lengths, from its shards in sorted (even j)
or shuffled (odd j) order.

Slivers come from the C restatement (erasure_patterns.encode), not from the engine's encode.
The output is one buffer of jobs * stride + 64 bytes, prefilled with a position-dependent
pattern and compared whole: source bytes below each job's length, the prefill everywhere else.
rs2_decode_batch_stats deltas must equal what erasure_patterns.batch_path predicts from the
layout alone.  All comparisons are exact.
"""
import numpy as np
import pytest
import torch

from erasure_patterns import (BATCH_CALLS, batch_jobs, batch_path, block_limit, decode_layout,
                              encode, families, load_cpu, odd_length, params, predicted_stats,
                              window_repeats)
from guarded import pattern

pytestmark = pytest.mark.gpu

OK, E_NOT_ENOUGH, E_UNSUCCESSFUL = 0, -5, -6
PREFILL = 90
TAIL = 64


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def stats():
    from walrus_amd.encoding import decode_batch_stats
    st = decode_batch_stats()
    return np.array([st["launches"], st["batched"], st["single"]], dtype=np.int64)


class BlobSet:
    """Four blobs of n shards and symbol size s with their slivers on the device (prim[b] = blob
    b's n primary slivers back to back, sec[b] likewise).  The lengths differ, so each job's cut
    at its blob's length does: the largest of the symbol size, odd_length (the middle of the
    last row) and two seeded odd lengths from the lower half of the symbol size's range (at
    s = 6 they end many rows earlier; at s = 130 the whole range is less than a row)."""

    def __init__(self, cpu, n, s, seed=0, lens=None):
        self.n, self.s = n, s
        self.kp, self.ks, _ = params(cpu, n, 1)
        full, lo = s * self.kp * self.ks, (s - 2) * self.kp * self.ks + 1
        if lens is None:
            rng = np.random.default_rng(n * 1000 + s)
            lens = [full, odd_length(cpu, n, s)]
            while len(lens) < 4:
                ln = int(rng.integers(lo, lo + (full - lo) // 2)) | 1
                if ln not in lens:
                    lens.append(ln)
            if s == 6:
                row = self.ks * s
                assert all(ln // row < lens[1] // row for ln in lens[2:])
        assert len(set(lens)) == 4 and max(lens) == full
        for ln in lens:
            assert params(cpu, n, ln) == (self.kp, self.ks, s)
        self.lens = list(lens)
        dev = torch.device("cuda", 0)
        enc = [encode(cpu, n, ln, seed=seed + 7000 + 10 * s + b) for b, ln in enumerate(lens)]
        self.blobs = [torch.from_numpy(e[0]).to(dev) for e in enc]
        self.prim = torch.from_numpy(np.stack([e[1].reshape(-1) for e in enc])).to(dev)
        self.sec = torch.from_numpy(np.stack([e[2].reshape(-1) for e in enc])).to(dev)
        self.stride = (full + 37) // 2 * 2

    def axis_of(self, k):
        assert k in (self.kp, self.ks)
        return "primary" if k == self.kp else "secondary"

    def slivers(self, axis):
        sl = self.prim if axis == "primary" else self.sec
        return sl, sl.shape[1] // self.n


_SETS = {}


def blob_set(cpu, n, s, seed=0, lens=None):
    """The shared, read-only blob set of (n, s, seed)."""
    if (n, s, seed) not in _SETS:
        _SETS[n, s, seed] = BlobSet(cpu, n, s, seed, lens)
    return _SETS[n, s, seed]


def fresh_output(bs, n_jobs):
    return pattern(n_jobs * bs.stride + TAIL, PREFILL, bs.prim.device)


def issue(plan, bs, axis, jobs, out, statuses=False, edit=None):
    """One batched call of `jobs` (batch_jobs) into `out`; `edit` may replace a job's selection."""
    sl, L = bs.slivers(axis)
    items, lens = [], []
    for j, (_, sel, b) in enumerate(jobs):
        sel = edit.get(j, sel) if edit else sel
        items.append((sel, [(b * bs.n + i) * L if i < bs.n else 0 for i in sel]))
        lens.append(bs.lens[b])
    st = torch.cuda.current_stream(sl.device).cuda_stream
    return plan.decode_batch_async(axis, items, sl.data_ptr(), out.data_ptr(), bs.stride, lens, st,
                                   statuses)


def expected(bs, jobs, skipped=(), blobs=None):
    want = fresh_output(bs, len(jobs))
    for j, (_, _, b) in enumerate(jobs):
        if j not in skipped:
            blob = (blobs or bs.blobs)[b]
            want[j * bs.stride:j * bs.stride + blob.numel()] = blob
    return want


def check(out, want, bs, jobs, lays, what):
    """The whole buffer; a mismatch names the job, its pattern and its layout."""
    torch.cuda.synchronize()
    if torch.equal(out, want):
        return
    bad = torch.nonzero(out != want).reshape(-1)
    o = int(bad[0])
    j = o // bs.stride
    if j >= len(jobs):
        raise AssertionError(f"{what}: {bad.numel()} wrong byte(s), the first at offset {o}, in "
                             f"the tail past the last job: got {int(out[o])} want {int(want[o])}")
    name, _, b = jobs[j]
    at = o - j * bs.stride
    where = "below" if at < bs.lens[b] else "at or past"
    raise AssertionError(
        f"{what}: {bad.numel()} wrong byte(s), the first at offset {o} = job {j} (pattern {name}, "
        f"blob {b} of {bs.lens[b]} bytes, {batch_path(lays[j], bs.s)}) byte {at}, {where} its "
        f"length: got {int(out[o])} want {int(want[o])}\n{lays[j]}")


def family_call(gpu, bs, k, limit, fams, may_fuse=True, statuses=False, edit=None):
    """One call of the family list `fams` at block limit `limit`, with a plan of its own:
    (out, jobs, layouts, stats delta, predicted stats, status codes)."""
    axis = bs.axis_of(k)
    jobs = batch_jobs(fams)
    lays = [decode_layout(k, bs.n, limit, sel) for _, sel, _ in jobs]
    out = fresh_output(bs, len(jobs))
    sl, _ = bs.slivers(axis)
    before_sl = sl.clone()
    with block_limit(limit):
        plan = gpu.DevicePlan(bs.n, max(bs.lens))
        assert plan.info.symbol_size == bs.s
        before = stats()
        codes = issue(plan, bs, axis, jobs, out, statuses, edit)
        torch.cuda.synchronize()
        delta = (stats() - before).tolist()
        del plan
    assert torch.equal(sl, before_sl), "the sliver buffer was written"
    return out, jobs, lays, delta, predicted_stats(lays, bs.s, may_fuse, set(edit or ())), codes


def assert_stats(delta, predicted, what):
    launches, batched, single = predicted
    assert delta[1:] == [batched, single], f"{what}: (launches, batched, single) = {delta}, " \
        f"predicted {predicted}"
    assert delta[0] >= launches, (what, delta, predicted)
    if not batched:
        assert delta[0] == 0, (what, delta)


def sizes_for(n):
    return (6, 66, 130) if n == 100 else (6,)


# ---- 1. one call per geometry and axis ---------------------------------------------------------
@pytest.mark.parametrize("k,n,limit,s", [
    pytest.param(k, n, limit, s, id=f"{k}of{n}-C{limit}-s{s}")
    for k, n, limit, _, _ in BATCH_CALLS for s in sizes_for(n)])
def test_families_one_call(gpu, cpu, k, n, limit, s):
    bs = blob_set(cpu, n, s)
    fams = families(k, n, limit)
    out, jobs, lays, delta, predicted, _ = family_call(gpu, bs, k, limit, fams)
    what = f"{k}-of-{n} block limit {limit} s={s} {bs.axis_of(k)}"
    print(f"{what}: {len(jobs)} jobs, (launches, batched, single) = {delta}")
    check(out, expected(bs, jobs), bs, jobs, lays, what)
    want = next(e for kk, nn, ll, _, e in BATCH_CALLS if (kk, nn, ll) == (k, n, limit))
    assert predicted == (1, want, len(fams) - want)
    assert_stats(delta, predicted, what)


# ---- 2. more than one planning window ------------------------------------------------------------
@pytest.mark.parametrize("order", ["family_order", "one_block_first"])
@pytest.mark.parametrize("k", [34, 67])
def test_two_windows(gpu, cpu, k, order):
    """The families repeated over the four blobs to more than 341 jobs: two planning windows, in
    family order (both as deep as the families go) and with every one-block job first (the first
    window launches one block deep, the second deeper)."""
    n, limit, s = 100, 16, 6
    bs = blob_set(cpu, n, s)
    fams = families(k, n, limit)
    fams = fams * window_repeats([decode_layout(k, n, limit, p) for _, p in fams])
    if order == "one_block_first":
        fams = sorted(fams, key=lambda f: len(decode_layout(k, n, limit, f[1]).out_blocks) != 1)
    out, jobs, lays, delta, predicted, _ = family_call(gpu, bs, k, limit, fams)
    what = f"{k}-of-{n} block limit {limit} s={s} {order}"
    check(out, expected(bs, jobs), bs, jobs, lays, what)
    assert predicted == (2, len(jobs), 0)
    assert_stats(delta, predicted, what)


# ---- 3. slot reuse ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [334, 667])
def test_back_to_back_calls_and_slot_memory(gpu, cpu, k):
    """Three calls with no synchronisation between them (two batch slots), a third of the
    families each, every call into its own buffer; then the first call again, at the same device
    addresses, with other blobs behind them: it must return the other blobs."""
    n, s, limit = 1000, 6, 512
    bs = blob_set(cpu, n, s)
    other = blob_set(cpu, n, s, seed=100, lens=bs.lens)
    axis = bs.axis_of(k)
    fams = families(k, n, limit)
    third = -(-len(fams) // 3)
    sl, _ = bs.slivers(axis)
    keep = sl.clone()
    calls = []
    with block_limit(limit):
        plan = gpu.DevicePlan(n, max(bs.lens))
        for c in range(3):
            jobs = batch_jobs(fams[c * third:(c + 1) * third], seed=c)
            out = fresh_output(bs, len(jobs))
            issue(plan, bs, axis, jobs, out)
            calls.append((jobs, out))
        assert sum(len(jobs) for jobs, _ in calls) == len(fams)
        for c, (jobs, out) in enumerate(calls):
            lays = [decode_layout(k, n, limit, sel) for _, sel, _ in jobs]
            check(out, expected(bs, jobs), bs, jobs, lays, f"{k}-of-{n} {axis} call {c}")
        assert torch.equal(sl, keep), "the sliver buffer was written"
        jobs, out = calls[0]
        try:
            sl.copy_(other.slivers(axis)[0])     # other blobs at the same addresses
            out.copy_(fresh_output(bs, len(jobs)))
            issue(plan, bs, axis, jobs, out)
            lays = [decode_layout(k, n, limit, sel) for _, sel, _ in jobs]
            check(out, expected(bs, jobs, blobs=other.blobs), bs, jobs, lays,
                  f"{k}-of-{n} {axis} call 0 again over other blobs")
        finally:
            torch.cuda.synchronize()
            sl.copy_(keep)
        del plan


# ---- 4. the status form -----------------------------------------------------------------------------
def test_statuses_in_a_heterogeneous_call(gpu, cpu):
    """(201, 300, 32) with every 10th job invalid -- one shard short on one, an index equal to n
    on the next: their codes as in test_gpu_decode_batch.test_errors_per_blob_and_whole_call,
    their output untouched, every other job exact, the counters over the valid jobs only."""
    k, n, limit, s = 201, 300, 32, 6
    bs = blob_set(cpu, n, s)
    fams = families(k, n, limit)
    jobs = batch_jobs(fams)
    edit, codes_want = {}, [OK] * len(jobs)
    for c, j in enumerate(range(9, len(jobs), 10)):
        sel = jobs[j][1]
        edit[j], codes_want[j] = ((sel[:-1], E_UNSUCCESSFUL) if c % 2 == 0 else
                                  ([n] + sel[1:], E_NOT_ENOUGH))
    assert len(edit) == 11
    out, jobs, lays, delta, predicted, codes = family_call(gpu, bs, k, limit, fams, statuses=True,
                                                           edit=edit)
    what = f"{k}-of-{n} block limit {limit} s={s} with statuses"
    assert codes == codes_want
    check(out, expected(bs, jobs, skipped=set(edit)), bs, jobs, lays, what)
    assert predicted[1] + predicted[2] == len(jobs) - len(edit) and predicted[2] > 0
    assert_stats(delta, predicted, what)
