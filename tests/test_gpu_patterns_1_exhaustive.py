"""Every erasure pattern of the small codes, byte for byte.

The codes are K_p / K_s of n_shards = 4, 7 and 10: (2,4), (3,4), (3,7), (5,7), (4,10), (7,10),
396 k-subsets in all.  Each subset is decoded

  * through the strided 1D codec (ops.decode_lines: rs2_codec_decode_device_async), with two
    and three lines, symbol sizes 2 (present originals go through the separate copy kernel) and
    6, at the default block limit and at limits 2 and 1 where they change C -- at limit 1,
    (7,10) is 16 blocks of one position -- so every mixing coefficient kind and every count /
    trunc of these codes occurs; the same body runs on the numpy oracle (unmarked, default
    limit: a block limit means nothing to it), which proves the body and the patterns first;
  * through the blob plan's decode (DevicePlan.decode_async: decode_device's destination layout,
    the cut at blob_len, the fused copy) on both axes, from slivers of the C restatement
    (oracle/rs2_cpu.c), into a buffer of blob_len bytes and a 64-byte pattern tail.

The expected bytes are the source data: nothing here comes from the engine's own encode.  All
comparisons are exact.  (This file sorts before test_gpu_patterns_2_structured.py on purpose:
the small codes run before n = 1000.)
"""
import pytest
import torch

from erasure_patterns import (SMALL, all_subsets, block_limit, check_blob, decode_layout, encode,
                              load_cpu, odd_length, params, run_patterns)
from guarded import ops_backend, pattern

SHAPES = ((2, 2), (3, 2), (2, 6), (3, 6))   # (lines, symbol size)


def _cases():
    out = []
    for k, n, limits in SMALL:
        out.append(pytest.param("cpu", k, n, None, id=f"cpu-{k}of{n}"))
        for b in limits:
            out.append(pytest.param("device", k, n, b, marks=pytest.mark.gpu,
                                    id=f"gpu-{k}of{n}-limit{b or 'default'}"))
    return out


@pytest.mark.parametrize("name,k,n,limit", _cases())
def test_every_subset_1d(request, name, k, n, limit):
    ops, device = ops_backend(name, request)
    subs = all_subsets(k, n)   # the subset of all sources included: copies only, no codec launch
    with block_limit(limit, apply=name == "device"):
        if name == "device":
            ops = type(ops)()   # codecs of this limit only
        for lines, s in SHAPES:
            on_erased, on_present = run_patterns(ops, device, k, n, limit, s, lines, subs)
            assert on_erased and on_present


# ---------------------------------------------------------------------------------------------
# the blob plan's decode
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


@pytest.mark.parametrize("s", [2, 6])
def test_lengths_are_odd_and_cut_the_last_row(cpu, s):
    for n in (4, 7, 10, 1000):
        odd_length(cpu, n, s)


@pytest.mark.gpu
@pytest.mark.parametrize("n,s,limit", [(n, s, None) for n in (4, 7, 10) for s in (2, 6)] +
                         [(10, 2, 1), (10, 6, 1)])
def test_every_subset_blob_plan(gpu, cpu, n, s, limit):
    dev = torch.device("cuda", 0)
    length = odd_length(cpu, n, s)
    blob, prim, sec = encode(cpu, n, length, seed=n * 100 + s)
    kp, ks, _ = params(cpu, n, length)
    pat = pattern(length + 64, 90, dev)
    want = torch.cat([torch.from_numpy(blob).to(dev), pat[length:]])
    buf = torch.empty_like(pat)
    st = torch.cuda.current_stream(dev).cuda_stream
    with block_limit(limit):
        plan = gpu.DevicePlan(n, length)
        for axis, k, sliv in (("primary", kp, prim), ("secondary", ks, sec)):
            src = torch.from_numpy(sliv.reshape(-1)).to(dev)
            before = src.clone()
            sl_len = sliv.shape[1]
            for name, sel in all_subsets(k, n):
                buf.copy_(pat)
                plan.decode_async(axis, sel, src.data_ptr(), [i * sl_len for i in sel],
                                  buf.data_ptr(), st)
                torch.cuda.synchronize()
                check_blob(buf, want, f"n={n} s={s} block limit {limit} {axis} from {sel}",
                           decode_layout(k, n, limit, sel))
            assert torch.equal(src, before), f"n={n} s={s} {axis}: slivers written"
        del plan
