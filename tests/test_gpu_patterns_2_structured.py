"""Structured erasure patterns (tests/erasure_patterns.py families) at the sizes that matter.

1D codec.  Each of the eight geometries -- (34,100) and (67,100) at block limit 16, (100,300)
and (200,300) at limit 64, (334,1000) and (667,1000) at limits 128 and 512; the limit forces
multi-block plans with several original blocks -- decodes every family pattern through
ops.decode_lines from oracle codewords (three lines, tight strides), with symbol sizes 2 (the
separate copy kernel) and 6, and 66 at n = 100, each pattern with out_limit beyond the buffer
and with an odd limit inside the last line whose cut symbol rotates over erased and present
originals.  The whole output buffer, a FILL tail included, is compared with the source symbols
below the limit and FILL from it on, the source buffer with its state before the call.  The
CPU leg (unmarked) runs the same body on the numpy oracle with one line, every fourth pattern at
n = 1000: every pattern is decodable by the reference alone, and the body is right before it
reaches a GPU.

Blob plan.  n = 1000 at the default limit: the families of (334,1000) on the primary axis and
of (667,1000) on the secondary axis through DevicePlan.decode_async, from slivers of the C
restatement, symbol sizes 2 and 6 (0.45 and 1.3 MB of blob).  A plan keeps two decode slots
and takes them in turn, each remembering the pattern (and addresses) it was planned for, so
each pattern is issued three times in a row at the same device addresses with another blob
behind them every time: the first two calls plan the pattern into either slot, the third runs
from the slot the first one planned and must return the third blob.

All comparisons are exact.
"""
import pytest
import torch

from erasure_patterns import (GEOMETRIES, block_limit, check_blob, decode_layout, encode, families,
                              load_cpu, odd_length, params, run_patterns)
from guarded import ops_backend, pattern


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def sizes_for(n):
    return (2, 6, 66) if n == 100 else (2, 6)


def _cases():
    out = []
    for k, n, limit, _ in GEOMETRIES:
        for s in sizes_for(n):
            out.append(pytest.param("cpu", k, n, limit, s, id=f"cpu-{k}of{n}-C{limit}-s{s}"))
            out.append(pytest.param("device", k, n, limit, s, marks=pytest.mark.gpu,
                                    id=f"gpu-{k}of{n}-C{limit}-s{s}"))
    return out


@pytest.mark.parametrize("name,k,n,limit,s", _cases())
def test_families_1d(request, name, k, n, limit, s):
    ops, device = ops_backend(name, request)
    fams = families(k, n, limit)
    lines = 3
    if name == "cpu":   # the oracle decodes a line at a time
        lines = 1
        fams = fams[::4] if n == 1000 else fams
    with block_limit(limit, apply=name == "device"):
        if name == "device":
            ops = type(ops)()   # codecs of this limit only
        on_erased, on_present = run_patterns(ops, device, k, n, limit, s, lines, fams)
    assert on_erased and on_present, "the cut never fell on an erased / a present original"


@pytest.fixture(scope="module", params=[2, 6], ids=lambda s: f"s{s}")
def blobs(request, cpu):
    """Three blobs of one odd length at n = 1000 with their slivers (C restatement)."""
    s = request.param
    length = odd_length(cpu, 1000, s)
    return s, length, [encode(cpu, 1000, length, seed=5000 + 10 * s + j) for j in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("axis", ["primary", "secondary"])
def test_families_blob_plan(gpu, cpu, blobs, axis):
    n = 1000
    s, length, enc = blobs
    kp, ks, _ = params(cpu, n, length)
    k = kp if axis == "primary" else ks
    dev = torch.device("cuda", 0)
    sliv = [torch.from_numpy(e[1 if axis == "primary" else 2].reshape(-1)).to(dev) for e in enc]
    sl_len = sliv[0].numel() // n
    pat = pattern(length + 64, 90, dev)
    want = [torch.cat([torch.from_numpy(e[0]).to(dev), pat[length:]]) for e in enc]
    src, buf = torch.empty_like(sliv[0]), torch.empty_like(pat)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan = gpu.DevicePlan(n, length)
    for name, sel in families(k, n, None):
        offs = [i * sl_len for i in sel]
        lay = decode_layout(k, n, None, sel)
        for j in range(3):   # the third call finds the slot the first one planned
            src.copy_(sliv[j])   # another blob at the same addresses
            buf.copy_(pat)
            plan.decode_async(axis, sel, src.data_ptr(), offs, buf.data_ptr(), st)
            torch.cuda.synchronize()
            check_blob(buf, want[j], f"n={n} s={s} {axis} pattern {name} call {j}", lay)
            assert torch.equal(src, sliv[j]), f"n={n} s={s} {axis} pattern {name}: slivers written"
    del plan
