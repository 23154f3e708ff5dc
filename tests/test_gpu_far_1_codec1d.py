"""The strided 1D device codec (rs2_codec_encode_device_async / rs2_codec_decode_device_async) at
far-apart lines and symbols: line strides on both sides of the planner's span switch and byte
offsets past 2^32.

The codec kernels address a symbol as a wave-uniform 64-bit base plus a 32-bit per-lane offset that
carries the lane's line step dl * line_stride.  finish_plan (rs2_planner.cpp) keeps that product
small: below T = (2^31 - 65536) / 64 = 33,553,408 bytes of line stride a line takes its pair count
rounded up to even in the flattened lane space (lanes of one 64-pair tile may sit on different
lines), from T on it takes a multiple of 64 (every tile lies in one line, dl == 0).  tests/
test_gpu_guard_codec1d.py runs line strides of a few hundred bytes; this file runs, for the same 14
codes (every block size C = 1 .. 512, both rates) and symbol sizes 2, 6, 66, 130 (1, 2, 17, 33
pairs per line: tiles of 32, 16, about 4 and about 2 lines under the even span),

  line stride T - 2, 3 and 34 lines   the last even span; at s = 2 and 34 lines tile 0 spans lines
                                      0 .. 31, the largest per-lane line step there is
  line stride T, 3 and 34 lines       the first 64-multiple span
  line stride 2^31 + 2, 3 lines       bit 31 set; the third line starts past 2^32

each on the source side alone, the destination side alone and both (the other side compact), and
symbol strides / symbol offsets of 2^31 + 2 under a compact line stride.  No test holds more than
5 GiB of device memory: a line stride of 2^31 + 2 makes a 4.3 GB buffer, so its "both sides far"
form is run one side at a time (that is, it is the source-alone and the destination-alone case and
nothing else), and tensors are dropped (and the allocator's cache emptied) before the next call.

Every call is described by `encode_calls` / `decode_calls` / `symbol_stride_calls` as plain data;
tests/test_planner_span.py hands the same descriptions to the planner on the CPU and asserts the
span each one gets.  The bodies are written against the `ops` interface (walrus_amd/partition.py)
and run twice: with tests/cpu_ops.CpuOps (unmarked, codes of k <= 34) with every far stride
divided by 2^12 and rounded to even -- that proves the layouts and the expected bytes against the
numpy oracle alone -- and with DeviceOps (-m gpu) at the real strides.  Per call:

  the written symbols equal rs2_oracle.rs_encode_symbols' / the codewords' source symbols;
  every byte of the output's windows (tests/far_buffers.py) outside the documented extents, and
  every byte at or past out_limit, keeps its pattern;
  the input's windows are unchanged.

In parametrisation order the T - 2 cases come before the T cases and those before the 2^31 ones.
"""
import numpy as np
import pytest
import torch

from far_buffers import WHOLE_MAX, FarBuffer, Grid
from guarded import ops_backend, sync as _sync
from test_gpu_guard_codec1d import PAIRS, _index_set, codewords

T = (2 ** 31 - 65536) // 64        # finish_plan: 64 * line stride + 65536 >= 2^31 from here on
FAR = 2 ** 31 + 2
SIZES = (2, 6, 66, 130)
# group -> [(line stride, lines)]
GROUPS = {"Tm2": [(T - 2, 3), (T - 2, 34)], "T": [(T, 3), (T, 34)], "2p31": [(FAR, 3)]}
SIDES = ("src", "dst", "both")
INDEX_SETS = ("fewest", "mix", "all")
LIMITS = ("beyond", "symend", "lastodd")
CPU_SCALE = 2 ** 12
CPU_MAX_K = 34
MAX_LINES = 34
BEYOND = 2 ** 64 - 1


def _far(v, scale, need):
    """A far stride: as it is on the device; divided by `scale` and rounded to even on the CPU,
    where a line longer than that ((34, 100) at s = 130: 8,580 bytes against 8,192) takes its own
    extent + 2 instead."""
    if scale == 1:
        assert v >= need
        return v
    return max(2 * round(v / (2 * scale)), need + 2)


def _limit(kind, k, s, lines, out_ss, out_ls):
    if kind == "symend":      # exactly at a symbol's end in the middle line
        return (lines // 2) * out_ls + (k // 2) * out_ss + s
    if kind == "lastodd":     # inside the last line's last symbol, at an odd byte
        return (lines - 1) * out_ls + (k - 1) * out_ss + s // 2
    return BEYOND


def _delta(*key):
    return 2 * (sum(int(x) for x in key) % 8)


def encode_calls(k, n, s, group, scale=1):
    r, si = n - k, SIZES.index(s)
    out = []
    for li, (ls, lines) in enumerate(GROUPS[group]):
        for di, side in enumerate(SIDES):
            if ls == FAR and side == "both":
                continue              # 2 x 4.3 GB: the two sides are run one at a time (above)
            src_ss, dst_ss = s + 2 * ((si + di) % 2), s + 2 * ((si + di + 1) % 2)
            src_ext, dst_ext = (k - 1) * src_ss + s, (r - 1) * dst_ss + s
            src_ls = _far(ls, scale, src_ext) if side != "dst" else src_ext + 10
            dst_ls = _far(ls, scale, dst_ext) if side != "src" else dst_ext + 2
            out.append(dict(op="enc", k=k, n=n, s=s, lines=lines, src_ss=src_ss, src_ls=src_ls,
                            dst_ss=dst_ss, dst_ls=dst_ls, delta=_delta(k, si, li, di),
                            tag=f"{group} x{lines} {side}"))
    return out


def decode_calls(k, n, s, group, scale=1):
    si = SIZES.index(s)
    rng = np.random.default_rng([n, k, s, list(GROUPS).index(group)])
    out, ci = [], 0
    for li, (ls, lines) in enumerate(GROUPS[group]):
        for di, side in enumerate(SIDES):
            if ls == FAR and side == "both":
                continue
            # out_limit matters where the destination is far (the stores' fast test and the fused
            # copy's limit test use dl_max * line stride): all three there, one otherwise
            for lim in (LIMITS if side != "src" else LIMITS[(si + li) % 3:][:1]):
                kind = INDEX_SETS[(ci + si + k) % 3]
                ci += 1
                idx = _index_set(kind, k, n, rng)
                src_ss, out_ss = s + 2 * ((si + ci) % 2), s + 2 * ((si + di) % 2)
                src_ext, out_ext = (len(idx) - 1) * src_ss + s, (k - 1) * out_ss + s
                src_ls = _far(ls, scale, src_ext) if side != "dst" else src_ext + 6
                out_ls = _far(ls, scale, out_ext) if side != "src" else out_ext + 2
                out.append(dict(op="dec", k=k, n=n, s=s, lines=lines, idx=idx,
                                sym_off=[j * src_ss for j in range(len(idx))], src_ls=src_ls,
                                out_ss=out_ss, out_ls=out_ls,
                                limit=_limit(lim, k, s, lines, out_ss, out_ls),
                                delta=_delta(k, si, li, di, ci),
                                tag=f"{group} x{lines} {side} idx={kind} limit={lim}"))
    return out


def symbol_stride_calls(s, scale=1):
    """Line stride compact (the lines of one symbol lie side by side), 3 lines, symbols 2^31 + 2
    apart: source position offsets up to 2^32 + 4 ((3, 7)), repair offsets likewise ((7, 10),
    r = 3), decode inputs at 0, 2^31 + 2 and 2^32 + 4 among small offsets, decode outputs
    2^31 + 2 apart (k = 3)."""
    si, lines, ls = SIZES.index(s), 3, s + 2
    far = _far(FAR, scale, (lines - 1) * ls + s)
    out = [dict(op="enc", k=3, n=7, s=s, lines=lines, src_ss=far, src_ls=ls, dst_ss=s,
                dst_ls=4 * s + 2, delta=_delta(si, 1), tag="src_sym_stride"),
           dict(op="enc", k=7, n=10, s=s, lines=lines, src_ss=s + 2, src_ls=7 * (s + 2) + 4,
                dst_ss=far, dst_ls=ls, delta=_delta(si, 2), tag="repair_sym_stride")]
    rng = np.random.default_rng([s, 99])
    blk = lines * ls                   # room for one entry's three lines
    idx = _index_set("mix", 7, 10, rng)
    off = [blk * (j // 2 + 1) if j % 2 == 0 else (far, 2 * far, 0)[j // 2] for j in range(7)]
    out.append(dict(op="dec", k=7, n=10, s=s, lines=lines, idx=idx, sym_off=off, src_ls=ls,
                    out_ss=s, out_ls=7 * s + 6, limit=BEYOND, delta=_delta(si, 3), tag="sym_off"))
    for ci, (kind, lim) in enumerate(zip(INDEX_SETS, LIMITS)):
        idx = _index_set(kind, 3, 7, rng)
        out.append(dict(op="dec", k=3, n=7, s=s, lines=lines, idx=idx,
                        sym_off=[j * (s + 2) for j in range(3)], src_ls=3 * (s + 2) + 2,
                        out_ss=far, out_ls=ls, limit=_limit(lim, 3, s, lines, far, ls),
                        delta=_delta(si, 4, ci), tag=f"out_sym_stride idx={kind} limit={lim}"))
    return out


def _runs(lines, ls, offs, s):
    """Where a buffer holds symbols: a run per line, or -- lines side by side under a far symbol
    stride -- a run per symbol position."""
    lo, ext = min(offs), max(offs) + s
    if ls >= ext - lo:
        return [(line * ls + lo, ext - lo) for line in range(lines)]
    return [(o, (lines - 1) * ls + s) for o in offs]


def _size(lines, ls, offs, s):
    return (lines - 1) * ls + max(offs) + s


def _dev(a, device):
    return torch.from_numpy(np.array(a, copy=True)).to(device)


def _fill(buf, lines, ls, offs, s, vals):
    """Symbol j of line l (vals[l][j]) to payload offset l * ls + offs[j]."""
    step = offs[1] - offs[0] if len(offs) > 1 else s
    if step >= s and all(o == offs[0] + j * step for j, o in enumerate(offs)):
        buf.payload[offs[0]:].as_strided((lines, len(offs), s), (ls, step, 1)).copy_(vals)
    else:
        for j, o in enumerate(offs):
            buf.payload[o:].as_strided((lines, s), (ls, 1)).copy_(vals[:, j])


def run_call(ops, device, c):
    k, n, s, lines = c["k"], c["n"], c["s"], c["lines"]
    what = " ".join(f"{key}={v}" for key, v in c.items() if key not in ("idx", "sym_off"))
    cw = codewords(k, n, s, MAX_LINES)[:lines]
    if c["op"] == "enc":
        src_offs = [i * c["src_ss"] for i in range(k)]
        src_ls, vals, want = c["src_ls"], cw[:, :k], cw[:, k:]
        grid = Grid(lines, c["dst_ls"], n - k, c["dst_ss"], s)
    else:
        src_offs, src_ls = c["sym_off"], c["src_ls"]
        vals, want = cw[:, c["idx"]], cw[:, :k]
        limit = c["limit"]
        grid = Grid(lines, c["out_ls"], k, c["out_ss"], s, None if limit == BEYOND else limit)
    src = FarBuffer(_size(lines, src_ls, src_offs, s), _runs(lines, src_ls, src_offs, s),
                    c["delta"], device, fill=17)
    _fill(src, lines, src_ls, src_offs, s, _dev(vals, device))
    snap = src.snapshot()
    dst_offs = [i * grid.strides[1] for i in range(grid.shape[1])]
    dst = FarBuffer(grid.size, _runs(lines, grid.strides[0], dst_offs, s),
                    (c["delta"] + 6) % 16, device, fill=90)
    assert src.total + dst.total < 5 << 30
    if c["op"] == "enc":
        ops.encode_lines(k, n, s, lines, src.payload, 0, c["src_ss"], src_ls,
                         dst.payload, 0, c["dst_ss"], c["dst_ls"])
    else:
        ops.decode_lines(k, n, s, lines, c["idx"], src.payload, src_offs, src_ls,
                         dst.payload, c["out_ss"], c["out_ls"], c["limit"])
    _sync(device)
    dst.assert_intact(grid, what)
    src.assert_unchanged(snap, what + ": input")
    got, want = dst.view(grid), _dev(want, device)
    if grid.limit is None:
        assert torch.equal(got, want), what
    else:
        at = (torch.arange(lines, device=device)[:, None, None] * grid.strides[0] +
              torch.arange(k, device=device)[None, :, None] * grid.strides[1] +
              torch.arange(s, device=device)[None, None, :])
        below = at < grid.limit
        assert bool(below.any()) and not bool(below.all()), what
        assert torch.equal(got[below], want[below]), what
    big = src.total + dst.total > WHOLE_MAX
    del src, dst, snap, got
    if big and torch.device(device).type == "cuda":
        torch.cuda.empty_cache()       # no 4.3 GB block is kept beside the next call's


def _params():
    out = []
    for group in GROUPS:               # T - 2 before T before 2^31
        for op in ("enc", "dec"):
            for k, n, c, rate in PAIRS:
                if k <= CPU_MAX_K:
                    out.append(pytest.param("cpu", op, group, k, n,
                                            id=f"cpu-{group}-{op}-{k}of{n}-C{c}{rate}"))
                out.append(pytest.param("device", op, group, k, n, marks=pytest.mark.gpu,
                                        id=f"gpu-{group}-{op}-{k}of{n}-C{c}{rate}"))
    return out


@pytest.mark.parametrize("name,op,group,k,n", _params())
def test_far_line_strides(request, name, op, group, k, n):
    ops, device = ops_backend(name, request)
    scale = CPU_SCALE if name == "cpu" else 1
    for s in SIZES:
        for c in (encode_calls if op == "enc" else decode_calls)(k, n, s, group, scale):
            run_call(ops, device, c)


@pytest.mark.parametrize("name,s", [pytest.param("cpu", s, id=f"cpu-s{s}") for s in SIZES] +
                         [pytest.param("device", s, marks=pytest.mark.gpu, id=f"gpu-s{s}")
                          for s in SIZES])
def test_far_symbol_strides(request, name, s):
    ops, device = ops_backend(name, request)
    for c in symbol_stride_calls(s, CPU_SCALE if name == "cpu" else 1):
        run_call(ops, device, c)


def test_calls_are_what_they_claim():
    """The case lists themselves (CPU): every code and size under every line case and side, the
    limits where their names say, offsets past 2^32 on the load and on the store side, and the
    tile that spans 32 lines."""
    assert T == 33_553_408 and 64 * (T - 2) + 65536 < 2 ** 31 <= 64 * T + 65536
    assert {c for _, _, c, _ in PAIRS} == {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}
    load_max = store_max = 0
    for k, n, _, _ in PAIRS:
        for s in SIZES:
            for group, cases in GROUPS.items():
                enc, dec = encode_calls(k, n, s, group), decode_calls(k, n, s, group)
                sides = 2 if group == "2p31" else 3
                assert len(enc) == len(cases) * sides
                assert len(dec) == len(cases) * (1 + 3 * (sides - 1))
                far = cases[0][0]
                assert {c["src_ls"] for c in enc + dec} > {far} and \
                    {c["dst_ls"] for c in enc} > {far} and {c["out_ls"] for c in dec} > {far}
                for c in enc:
                    assert min(c["src_ss"], c["dst_ss"]) >= s and c["src_ls"] >= k * s
                    load_max = max(load_max, (c["lines"] - 1) * c["src_ls"])
                    store_max = max(store_max, (c["lines"] - 1) * c["dst_ls"])
                for c in dec:
                    used = [q for q in dict.fromkeys(c["idx"]) if q < n][:k]
                    assert len(used) == k == len(c["idx"])
                    lim, ols, oss = c["limit"], c["out_ls"], c["out_ss"]
                    if "limit=symend" in c["tag"]:
                        assert lim // ols == c["lines"] // 2 and (lim % ols - s) % oss == 0
                        assert s <= lim % ols <= (k - 1) * oss + s
                    if "limit=lastodd" in c["tag"]:
                        assert lim % 2 == 1 and lim // ols == c["lines"] - 1
                        assert 0 < lim - (c["lines"] - 1) * ols - (k - 1) * oss < s
                    load_max = max(load_max, (c["lines"] - 1) * c["src_ls"])
                    store_max = max(store_max, (c["lines"] - 1) * ols)
                if group != "2p31":    # all three index sets and limits meet a far destination
                    far_dst = [c["tag"] for c in dec if " src " not in c["tag"]]
                    assert all(any(f"limit={lim}" in t for t in far_dst) for lim in LIMITS)
            tags = {c["tag"].split(" idx=")[1] for g in GROUPS for c in decode_calls(k, n, s, g)}
            assert {t.split(" ")[0] for t in tags} == set(INDEX_SETS)
    assert load_max > 2 ** 32 and store_max > 2 ** 32
    # one tile of 64 pairs at s = 2 (one pair per line, span 2): lines 0 .. 31 of the 34
    assert (T - 2, 34) in GROUPS["Tm2"] and 64 // 2 <= 34 and 31 * (T - 2) < 2 ** 31
    for s in SIZES:
        sym = symbol_stride_calls(s)
        assert [c["tag"].split(" ")[0] for c in sym] == ["src_sym_stride", "repair_sym_stride",
                                                         "sym_off"] + ["out_sym_stride"] * 3
        assert sym[0]["src_ss"] == FAR and 2 * FAR == 2 ** 32 + 4 and sym[1]["dst_ss"] == FAR
        assert {0, FAR, 2 * FAR} < set(sym[2]["sym_off"]) and \
            sum(o < 2 ** 16 for o in sym[2]["sym_off"]) == 5
        assert all(c["out_ss"] == FAR for c in sym[3:])
        # symbols of different entries never overlap (Grid checks the outputs)
        ext = sorted((o, o + 2 * sym[2]["src_ls"] + s) for o in sym[2]["sym_off"])
        assert all(a[1] <= b[0] for a, b in zip(ext, ext[1:]))


@pytest.mark.gpu
def test_strides_and_offsets_of_2_to_47_are_refused(gpu):
    """include/walrus_rs2.h: every stride and sym_off of the codec calls is below 2^47; a larger
    one is RS2_E_INVALID_ARGUMENT.  Asked with lines = 0 only, where a call that passes the checks
    returns RS2_OK without planning or launching anything."""
    import ctypes
    from walrus_amd import _lib
    L = _lib.lib()
    INVALID, BIG, OK_MAX = _lib.RS2_E_INVALID_ARGUMENT, 2 ** 47, 2 ** 47 - 2
    k, n, s = 4, 10, 6
    codec = ctypes.c_void_p()
    assert L.rs2_codec_create(k, n, s, ctypes.byref(codec)) == 0
    try:
        def enc(ss=s, ls=k * s, rs=s, rl=(n - k) * s):
            return L.rs2_codec_encode_device_async(codec, 0, None, ss, ls, None, rs, rl, None)

        def dec(off=(0, 6, 12, 18), ls=n * s, oss=s, ols=k * s, idx=(4, 5, 6, 7)):
            return L.rs2_codec_decode_device_async(
                codec, 0, len(idx), (ctypes.c_uint16 * len(idx))(*idx), None,
                (ctypes.c_uint64 * len(off))(*off), ls, None, oss, ols, 2 ** 64 - 1, None)

        ok = [enc(), dec(), enc(ss=OK_MAX), enc(ls=OK_MAX), enc(rs=OK_MAX), enc(rl=OK_MAX),
              dec(off=(0, 6, OK_MAX, 18)), dec(ls=OK_MAX), dec(oss=OK_MAX), dec(ols=OK_MAX)]
        assert ok == [0] * len(ok), (ok, _lib.last_error())
        for big in (BIG, BIG + 2, 2 ** 63, 2 ** 64 - 2):
            rcs = [enc(ss=big), enc(ls=big), enc(rs=big), enc(rl=big),
                   dec(off=(0, 6, big, 18)), dec(ls=big), dec(oss=big), dec(ols=big),
                   # the offset of an ignored entry (an index >= n_shards) is checked like the rest
                   dec(off=(0, 6, 12, 18, big), idx=(4, 5, 6, 7, 99))]
            assert rcs == [INVALID] * len(rcs), (big, rcs)
    finally:
        L.rs2_codec_destroy(codec)
