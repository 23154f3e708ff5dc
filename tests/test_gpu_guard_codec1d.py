"""The strided 1D device codec (rs2_codec_encode_device_async / rs2_codec_decode_device_async,
the whole compute path of the partitioned multi-GPU code) inside guard bands.

The bodies are written against the `ops` interface of walrus_amd/partition.py (encode_lines,
decode_lines) and run twice: with tests/cpu_ops.CpuOps on CPU tensors (unmarked: validates the
test logic, the layouts and the expected bytes against the numpy oracle alone; codes of
k <= 34, fewer lines and placements, since the oracle decodes a line at a time) and with
DeviceOps on the GPU (-m gpu).  Every buffer has exactly its documented extent (no slack) and
lies in the interior of a tests/guarded.Guarded allocation; for every case and every placement
`delta` (the buffers' residue mod 16):

  A  containment   the guards of the output and every gap between its symbols / lines, and
                   every byte at or past out_limit, keep their pattern; the input is unchanged
  B  independence  the same call with another fill of the input's guards and gaps gives a
                   bit-identical output buffer
  C  correctness   the written symbols equal rs2_oracle.rs_encode_symbols / the codewords'
                   source symbols (what rs_decode_symbols returns; the CPU run decodes with it)

  basic_encoding.rs:195-211 encode_all      basic_encoding.rs:387-429 decode
"""
import numpy as np
import pytest
import torch

import rs2_oracle as O
from guarded import DELTAS, Guarded, ops_backend, strided_mask, sync as _sync

# (k, n_shards, C, rate): the transform block C (one kernel geometry each, rs2_engine.cpp
# launch_codec_c: C = 1 .. 512) and the rate plan_encode / plan_decode pick for the pair:
#   high rate iff pow2(n - k) <= pow2(k);  chunk = pow2(n - k) if high else pow2(k);
#   C = min(chunk, 512), the same on the encode and the decode side
PAIRS = [
    (1, 2, 1, "high"), (2, 4, 2, "high"), (3, 7, 4, "high"), (4, 10, 4, "low"),
    (7, 10, 4, "high"), (11, 19, 8, "high"), (13, 40, 16, "low"), (27, 50, 32, "high"),
    (34, 100, 64, "low"), (67, 100, 64, "high"), (100, 300, 128, "low"),
    (300, 450, 256, "high"), (334, 1000, 512, "low"), (667, 1000, 512, "high"),
]
SIZES = (2, 6, 64, 66, 130)
LINES = (1, 3, 65)
CPU_LINES = (1, 2, 3)       # the oracle behind CpuOps works a line at a time
CPU_DELTAS = (6,)
CPU_MAX_K = 34
INDEX_SETS = ("all", "fewest", "mix", "dups", "oob")
LIMITS = ("zero", "mid0", "symend", "lastline", "beyond")


def _pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def geometry(k, n):
    """The planner's choice restated (plan_encode / plan_decode): (C, rate)."""
    r = n - k
    high = _pow2(r) <= _pow2(k)
    return min(_pow2(r) if high else _pow2(k), 512), "high" if high else "low"


def test_pairs_reach_every_kernel_geometry():
    assert all(geometry(k, n) == (c, rate) for k, n, c, rate in PAIRS)
    assert {c for _, _, c, _ in PAIRS} == {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}
    for must in [(1, 2), (2, 4), (3, 7), (4, 10), (7, 10), (34, 100), (67, 100), (334, 1000),
                 (667, 1000)]:
        assert must in [(k, n) for k, n, _, _ in PAIRS]
    for k, n, _, _ in PAIRS:   # every code is one rs2_codec_create accepts
        r = n - k
        assert 0 < k < n and min(_pow2(k), _pow2(r)) + max(k, r) <= 65536


_REF = {}


def codewords(k, n, s, lines):
    """`lines` codewords of the (k, n) code: [lines][n][s] bytes, source || repair, from the
    oracle.  Computed once per (k, n, s) and shared (read-only) by both backends."""
    key = (k, n, s)
    if key not in _REF or _REF[key].shape[0] < lines:
        rng = np.random.default_rng(k * 1_000_003 + n * 1009 + s)
        data = rng.integers(0, 256, (lines, k, s), dtype=np.uint8)
        rep = np.stack([O.rs_encode_symbols(data[i], n - k) for i in range(lines)])
        cw = np.concatenate([data, rep], axis=1)
        cw.setflags(write=False)
        _REF[key] = cw
    return _REF[key][:lines]


def _grid(lines, line_stride, symbols, sym_stride, s):
    return (np.arange(lines, dtype=np.int64)[:, None, None] * line_stride +
            np.arange(symbols, dtype=np.int64)[None, :, None] * sym_stride +
            np.arange(s, dtype=np.int64)[None, None, :])


def _size(lines, line_stride, symbols, sym_stride, s):
    """Exact extent of a strided buffer: up to the last byte of the last line's last symbol."""
    return (lines - 1) * line_stride + (symbols - 1) * sym_stride + s


def _t(a, device):
    return torch.from_numpy(np.array(a, copy=True)).to(device)


def _strides(s):
    return (s, s + 2, s + 30)


def run_encode(ops, device, k, n, s, lines_set, deltas):
    r = n - k
    ss = _strides(s)
    for ci, lines in enumerate(lines_set):
        cw = codewords(k, n, s, max(lines_set))[:lines]
        src_ss, dst_ss, gap = ss[ci % 3], ss[(ci + 2) % 3], (2, 10, 34)[ci % 3]
        src_ls = (k - 1) * src_ss + s + gap
        dst_ls = (r - 1) * dst_ss + s + gap
        src_size, dst_size = _size(lines, src_ls, k, src_ss, s), _size(lines, dst_ls, r, dst_ss, s)
        sgrid = _t(_grid(lines, src_ls, k, src_ss, s).reshape(-1), device)
        svals = _t(cw[:, :k].reshape(-1), device)
        dmask = strided_mask(dst_size, lines, dst_ls, r, dst_ss, s)
        dgrid = _t(_grid(lines, dst_ls, r, dst_ss, s).reshape(-1), device)
        want = _t(cw[:, k:].reshape(-1), device)
        for delta in deltas:
            what = (f"encode k={k} n={n} s={s} lines={lines} src stride {src_ss}/{src_ls} "
                    f"dst stride {dst_ss}/{dst_ls} delta={delta}")
            outs = []
            for fill in (17, 201):
                src = Guarded(src_size, delta, device, fill)
                src.payload[sgrid] = svals
                before = src.buf.clone()
                dst = Guarded(dst_size, (delta + 4 * ci) % 16, device, fill=90)
                ops.encode_lines(k, n, s, lines, src.payload, 0, src_ss, src_ls,
                                 dst.payload, 0, dst_ss, dst_ls)
                _sync(device)
                dst.assert_guards_intact(dmask, what)                      # A
                assert torch.equal(src.buf, before), what + ": input written"
                assert torch.equal(dst.payload[dgrid], want), what         # C
                outs.append(dst.buf)
            assert torch.equal(outs[0], outs[1]), what + ": output depends on bytes outside the input"  # B


def _index_set(kind, k, n, rng):
    """Shard indices of a decode call (k distinct valid ones among them)."""
    r = n - k
    if kind == "all":        # every source present: copies only, no codec launch
        return [int(i) for i in rng.permutation(k)]
    if kind == "fewest":     # every repair shard, as few sources as the code allows (none if r >= k)
        return list(range(k, n))[:k] + list(range(k - 1, -1, -1))[:max(0, k - r)]
    mix = [int(i) for i in rng.permutation(n)[:k]]
    if all(i < k for i in mix):   # make sure a repair shard takes part
        mix[0] = k
        mix = list(dict.fromkeys(mix))
        mix += [i for i in range(k) if i not in mix][:k - len(mix)]
    if kind == "mix":
        return mix
    if kind == "dups":       # repeats of earlier entries in between (ignored)
        return mix[:1] + mix[:1] + mix[1:] + mix[:2]
    assert kind == "oob"     # one index >= n_shards in the list (ignored per the header)
    return mix[:k // 2] + [n + 3] + mix[k // 2:]


def _limit(kind, k, s, lines, out_ss, out_ls, size):
    if kind == "zero":
        return 0
    if kind == "mid0":       # inside a symbol of line 0, odd where the symbol has room for it
        return min(1, k - 1) * out_ss + (s // 2 + 1 if s > 2 else 1)
    if kind == "symend":     # exactly at a symbol's end
        return min(1, lines - 1) * out_ls + (k // 2) * out_ss + s
    if kind == "lastline":   # inside the last line's last symbol
        return (lines - 1) * out_ls + (k - 1) * out_ss + (s // 2 - 1 if s > 2 else 1)
    return 2 ** 64 - 1       # beyond the end: nothing is cut


def run_decode(ops, device, k, n, s, lines_set, deltas):
    ss = _strides(s)
    rng = np.random.default_rng(n * 131 + k * 7 + s)
    ci = 0
    for kind in INDEX_SETS:
        for lim_kind in LIMITS:
            lines = lines_set[(ci + ci // 5) % 3]
            cw = codewords(k, n, s, max(lines_set))[:lines]
            src_ss, out_ss, gap = ss[ci % 3], ss[(ci // 3) % 3], (2, 10, 34)[(ci // 2) % 3]
            src_ls = (n - 1) * src_ss + s + gap
            out_ls = (k - 1) * out_ss + s + gap
            src_size = _size(lines, src_ls, n, src_ss, s)
            out_size = _size(lines, out_ls, k, out_ss, s)
            idx = _index_set(kind, k, n, rng)
            sym_off = [(q if q < n else 0) * src_ss for q in idx]
            limit = _limit(lim_kind, k, s, lines, out_ss, out_ls, out_size)
            sgrid = _t(_grid(lines, src_ls, n, src_ss, s).reshape(-1), device)
            svals = _t(cw.reshape(-1), device)
            omask = strided_mask(out_size, lines, out_ls, k, out_ss, s, limit)
            full = np.zeros(out_size, dtype=np.uint8)
            full[_grid(lines, out_ls, k, out_ss, s).reshape(-1)] = cw[:, :k].reshape(-1)
            ogrid = _t(np.flatnonzero(omask), device)
            want = _t(full[omask], device)
            for delta in deltas:
                what = (f"decode k={k} n={n} s={s} lines={lines} idx={kind} limit={lim_kind}"
                        f"({limit}) src stride {src_ss}/{src_ls} out stride {out_ss}/{out_ls} "
                        f"delta={delta}")
                outs = []
                for fill in (17, 201):
                    src = Guarded(src_size, delta, device, fill)
                    src.payload[sgrid] = svals
                    before = src.buf.clone()
                    out = Guarded(out_size, (delta + 2 * ci) % 16, device, fill=90)
                    ops.decode_lines(k, n, s, lines, idx, src.payload, sym_off, src_ls,
                                     out.payload, out_ss, out_ls, limit)
                    _sync(device)
                    out.assert_guards_intact(omask, what)                   # A
                    assert torch.equal(src.buf, before), what + ": input written"
                    assert torch.equal(out.payload[ogrid], want), what      # C
                    outs.append(out.buf)
                assert torch.equal(outs[0], outs[1]), \
                    what + ": output depends on bytes outside the input"    # B
            ci += 1


def _backends():
    out = []
    for k, n, c, rate in PAIRS:
        for s in SIZES:
            if k <= CPU_MAX_K:
                out.append(pytest.param("cpu", k, n, s, id=f"cpu-{k}of{n}-C{c}{rate}-s{s}"))
            out.append(pytest.param("device", k, n, s, marks=pytest.mark.gpu,
                                    id=f"gpu-{k}of{n}-C{c}{rate}-s{s}"))
    return out


def _backend(name, request):
    ops, device = ops_backend(name, request)
    return (ops, device) + ((CPU_LINES, CPU_DELTAS) if name == "cpu" else (LINES, DELTAS))


@pytest.mark.parametrize("name,k,n,s", _backends())
def test_encode_lines_guarded(request, name, k, n, s):
    ops, device, lines_set, deltas = _backend(name, request)
    run_encode(ops, device, k, n, s, lines_set, deltas)


@pytest.mark.parametrize("name,k,n,s", _backends())
def test_decode_lines_guarded(request, name, k, n, s):
    ops, device, lines_set, deltas = _backend(name, request)
    run_decode(ops, device, k, n, s, lines_set, deltas)


def test_index_sets_and_limits_are_what_they_claim():
    """The decode cases themselves (CPU): k distinct valid indices in every set, the special
    entries present, and each limit where its name says."""
    rng = np.random.default_rng(0)
    for k, n, _, _ in PAIRS:
        for kind in INDEX_SETS:
            idx = _index_set(kind, k, n, rng)
            valid = list(dict.fromkeys(i for i in idx if i < n))
            assert len(valid) >= k, (k, n, kind)
            used = valid[:k]
            if kind == "all":
                assert sorted(used) == list(range(k))
            if kind == "fewest":
                assert sum(i < k for i in used) == max(0, 2 * k - n)
            if kind in ("mix", "dups", "oob"):
                assert any(i >= k for i in used)
            if kind == "dups":
                assert len(idx) > len(set(idx))
            if kind == "oob":
                assert sum(i >= n for i in idx) == 1
        for s in SIZES:
            for lines in LINES:
                out_ss, out_ls = s + 2, (k - 1) * (s + 2) + s + 10
                size = _size(lines, out_ls, k, out_ss, s)
                lim = {kind: _limit(kind, k, s, lines, out_ss, out_ls, size) for kind in LIMITS}
                assert lim["zero"] == 0 and lim["beyond"] > size
                assert 0 < lim["mid0"] % out_ss < s and lim["mid0"] < out_ls
                assert (lim["symend"] % out_ls) % out_ss == s and lim["symend"] <= size
                assert size - s < lim["lastline"] < size


@pytest.mark.gpu
def test_codec_calls_reject_misaligned_arguments(gpu):
    """include/walrus_rs2.h: codec sources and destinations, every symbol offset and all strides
    are 2-byte aligned; a violation is RS2_E_INVALID_ARGUMENT on the host and nothing is
    enqueued: the buffers stay as they were."""
    import ctypes
    from walrus_amd import _lib
    L = _lib.lib()
    INVALID = _lib.RS2_E_INVALID_ARGUMENT
    k, n, s = 4, 10, 6
    codec = ctypes.c_void_p()
    assert L.rs2_codec_create(k, n, s, ctypes.byref(codec)) == 0
    try:
        dev = torch.device("cuda", 0)
        buf = torch.full((1 << 14,), 0x5A, dtype=torch.uint8, device=dev)
        a, b = buf.data_ptr(), buf.data_ptr() + 8192
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def enc(src=a, ss=s, ls=k * s, dst=b, rs=s, rl=(n - k) * s):
            return L.rs2_codec_encode_device_async(codec, 2, src, ss, ls, dst, rs, rl, st)

        def dec(base=a, off=(0, 6, 12, 18), ls=n * s, out=b, oss=s, ols=k * s, idx=(4, 5, 6, 7)):
            return L.rs2_codec_decode_device_async(
                codec, 2, len(idx), (ctypes.c_uint16 * len(idx))(*idx), base,
                (ctypes.c_uint64 * len(off))(*off), ls, out, oss, ols, 2 ** 64 - 1, st)

        rcs = [enc(src=a + 1), enc(ss=s + 1), enc(ls=k * s + 1), enc(dst=b + 1), enc(rs=s + 1),
               enc(rl=(n - k) * s + 1),
               dec(base=a + 1), dec(off=(0, 6, 13, 18)), dec(ls=n * s + 1), dec(out=b + 1),
               dec(oss=s + 1), dec(ols=k * s + 1),
               # the offset of an ignored entry (an index >= n_shards) is checked like the rest
               dec(off=(0, 6, 12, 18, 3), idx=(4, 5, 6, 7, 99))]
        assert rcs == [INVALID] * len(rcs), rcs
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all()), "a refused call wrote to its buffers"
    finally:
        L.rs2_codec_destroy(codec)
