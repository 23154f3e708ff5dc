"""Sparse guard-band buffers for strided layouts of gigabytes -- TEST ONLY (a plain module, no
fixtures).

tests/guarded.Guarded fills and scans a whole allocation, which does not scale to lines that lie
32 MiB or 2 GiB apart.  A `FarBuffer` is one owned uint8 allocation of GUARD + delta + size + GUARD
bytes, allocated UNINITIALISED; the payload (what a kernel is handed) sits in its interior, `delta`
being its residue mod 16 as in Guarded.  The caller names the payload's `runs`, the (offset, length)
stretches that hold symbols (one per line for a far line stride, one per symbol for a far symbol
stride: see `line_runs`).  The position-dependent pattern of guarded.pattern is laid over every run
plus 4 KiB on each side, clipped to the allocation and merged where such windows meet; the guards
are windows of their own.  After the call, `changed()` / `assert_intact()` report every window
byte that is not a documented output byte (a `Grid`, cut at its out_limit) and no longer holds the
pattern.  A stray write further than 4 KiB from every run goes unseen in a sparse buffer; so
allocations of up to 1.25 GiB (WHOLE_MAX) are filled and compared whole, the bytes between the
windows included, in chunks of 16 MiB so that no temporary exceeds 256 MiB.

The same class serves CPU tensors (device="cpu"), whose payload tests/cpu_ops.CpuOps takes as it
takes a Guarded one.  Reads outside the runs are not detected here."""
import numpy as np
import torch

GUARD = 4096
WHOLE_MAX = 5 << 28          # 1.25 GiB: allocations up to this size are filled and checked whole
CHUNK = 1 << 24              # bytes handled per step (the int64 ramp behind the pattern: 128 MiB)

_BASE = {}


def _pattern(a, b, fill, device):
    """Bytes a .. b of guarded.pattern ((i*131 + fill) & 0xFF, period 256), b - a <= CHUNK."""
    key = (str(device), int(fill))
    if key not in _BASE:
        i = torch.arange(CHUNK + 256, dtype=torch.int64, device=device)
        _BASE[key] = ((i * 131 + int(fill)) & 0xFF).to(torch.uint8)
    assert 0 <= b - a <= CHUNK
    return _BASE[key][(a & 255):(a & 255) + (b - a)]


def _chunks(a, b):
    while a < b:
        yield a, min(a + CHUNK, b)
        a += CHUNK


def line_runs(lines, line_stride, run_len):
    """One run of run_len bytes per line."""
    return [(line * line_stride, run_len) for line in range(lines)]


def merge_windows(runs, lo, hi, pad=GUARD):
    """The runs widened by `pad` on each side, clipped to [lo, hi) and merged where they touch or
    overlap: sorted, disjoint [(begin, end)]."""
    out = []
    for off, ln in sorted((int(o), int(n)) for o, n in runs):
        a, b = max(off - pad, lo), min(off + ln + pad, hi)
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


class Grid:
    """The documented output bytes of a strided call: lines x symbols symbols of s bytes at
    line * line_stride + i * sym_stride, cut at payload offset `limit` (bytes at or past it are
    not written).  Symbols must not overlap."""

    def __init__(self, lines, line_stride, symbols, sym_stride, s, limit=None):
        self.shape = (int(lines), int(symbols), int(s))
        self.strides = (int(line_stride), int(sym_stride))
        self.s = int(s)
        self.limit = None if limit is None else int(limit)
        st = (np.arange(lines, dtype=np.int64)[:, None] * int(line_stride) +
              np.arange(symbols, dtype=np.int64)[None, :] * int(sym_stride)).reshape(-1)
        self.starts = np.sort(st)
        assert self.starts.size < 2 or int(np.diff(self.starts).min()) >= self.s, "symbols overlap"
        self.size = int(self.starts[-1]) + self.s if st.size else 0

    def mask(self, lo, hi):
        """Boolean numpy mask over payload offsets lo .. hi: True = may be written."""
        a = np.searchsorted(self.starts, lo - self.s, side="right")
        b = np.searchsorted(self.starts, hi, side="left")
        st = self.starts[a:b]
        en = st + self.s
        if self.limit is not None:
            en = np.minimum(en, self.limit)
        begin = np.clip(st, lo, hi) - lo
        end = np.maximum(np.clip(en, lo, hi) - lo, begin)
        d = np.zeros(hi - lo + 1, dtype=np.int32)
        np.add.at(d, begin, 1)
        np.add.at(d, end, -1)
        return np.cumsum(d[:-1]) > 0

    def where(self, at):
        """What kind of byte payload offset `at` is (for messages)."""
        i = int(np.searchsorted(self.starts, at, side="right")) - 1
        if i >= 0 and at < int(self.starts[i]) + self.s:
            return "at or past out_limit" if self.limit is not None and at >= self.limit \
                else "a writable byte"
        return "gap between the writable extents"


class FarBuffer:
    def __init__(self, size, runs, delta=0, device="cpu", fill=0, whole=None):
        self.size, self.delta, self.fill = int(size), int(delta), int(fill)
        self.start = GUARD + self.delta
        self.total = self.start + self.size + GUARD
        for off, ln in runs:
            assert 0 <= off and off + ln <= self.size, "run outside the payload"
        self.buf = torch.empty(self.total, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0, "allocation is not 16-byte aligned"
        self.payload = self.buf[self.start:self.start + self.size]
        self.ptr = self.buf.data_ptr() + self.start
        # windows in payload coordinates; the guards belong to the first and the last one or
        # stand alone (a zero-length run at each end of the payload)
        self.windows = merge_windows(list(runs) + [(-self.delta, self.delta), (self.size, 0)],
                                     -self.start, self.size + GUARD)
        # whole: overrides the size rule (the helper's own test runs both forms at small sizes)
        self.whole = self.total <= WHOLE_MAX if whole is None else bool(whole)
        for a, b in self._regions():
            self.buf[a:b] = _pattern(a, b, self.fill, self.buf.device)

    def _regions(self):
        """Allocation ranges that hold the pattern, in chunks."""
        if self.whole:
            yield from _chunks(0, self.total)
        else:
            for lo, hi in self.windows:
                yield from _chunks(lo + self.start, hi + self.start)

    def view(self, grid):
        """The grid's symbols as a [lines][symbols][s] strided view of the payload."""
        assert grid.size <= self.size
        return self.payload.as_strided(grid.shape, grid.strides + (1,))

    def snapshot(self):
        """Copies of the windows (an input's state before the call)."""
        return [self.buf[lo + self.start:hi + self.start].clone() for lo, hi in self.windows]

    def assert_unchanged(self, snap, what="input"):
        for (lo, hi), was in zip(self.windows, snap):
            now = self.buf[lo + self.start:hi + self.start]
            if not torch.equal(now, was):
                at = int(torch.nonzero(now != was)[0]) + lo
                raise AssertionError(f"{what}: written at payload offset {at}")

    def changed(self, grid=None):
        """Payload offsets (front guard negative), ascending, of the bytes that must keep the
        pattern and did not: every window byte that `grid` (None: no byte at all) does not
        document as output, and in a whole buffer every byte between the windows too."""
        dev = self.buf.device
        bad = []
        covered = {}
        for lo, hi in self.windows:
            keep = ~grid.mask(lo, hi) if grid is not None else np.ones(hi - lo, dtype=bool)
            for a, b in _chunks(lo + self.start, hi + self.start):
                k = torch.from_numpy(keep[a - lo - self.start:b - lo - self.start]).to(dev)
                ne = (self.buf[a:b] != _pattern(a, b, self.fill, dev)) & k
                if bool(ne.any()):
                    bad += (torch.nonzero(ne).reshape(-1) + (a - self.start)).cpu().tolist()
            covered[lo + self.start] = hi + self.start
        if self.whole:
            at = 0
            for lo in sorted(covered) + [self.total]:
                for a, b in _chunks(at, lo):
                    ne = self.buf[a:b] != _pattern(a, b, self.fill, dev)
                    if bool(ne.any()):
                        bad += (torch.nonzero(ne).reshape(-1) + (a - self.start)).cpu().tolist()
                at = covered.get(lo, lo)
        return sorted(bad)

    def assert_intact(self, grid=None, what="buffer"):
        bad = self.changed(grid)
        if bad:
            at = bad[0]
            where = ("front guard" if at < 0 else "back guard" if at >= self.size else
                     grid.where(at) if grid is not None else "payload")
            raise AssertionError(
                f"{what}: {len(bad)} byte(s) outside the writable extent changed, the first at "
                f"payload offset {at} ({where}; payload {self.size} bytes, delta {self.delta}, "
                f"{'whole' if self.whole else 'windows only'})")
