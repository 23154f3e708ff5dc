"""Guard-band buffers for the containment tests -- TEST ONLY (a plain module, no fixtures).

A `Guarded` buffer is one owned uint8 allocation of GUARD + delta + size + GUARD bytes filled
with a position-dependent pattern.  The payload (what a kernel is handed) sits in its interior:
`delta` moves it off the allocation's alignment (the allocation itself is at least 16-byte
aligned, so `delta` is the payload's residue mod 16), and 4 KiB of pattern lie on each side, so
everything a slightly wrong kernel can touch is memory this buffer owns.  After the call,
`assert_guards_intact()` compares both guards -- and, for strided outputs, every payload byte
outside the extents that may be written -- with the pattern and names the first changed byte.

Reads outside the payload are not detected here; they show in results only (run the same call
with another guard `fill` on the inputs and compare the outputs bit for bit).
"""
import numpy as np
import torch

GUARD = 4096
DELTAS = (0, 2, 4, 6, 8, 10, 12, 14)


def pattern(total, fill, device="cpu"):
    """Byte i of the pattern seeded by `fill`: (i*131 + fill) & 0xFF."""
    i = torch.arange(total, dtype=torch.int64, device=device)
    return ((i * 131 + int(fill)) & 0xFF).to(torch.uint8)


class Guarded:
    def __init__(self, size, delta=0, device="cpu", fill=0):
        self.size, self.delta, self.fill = int(size), int(delta), int(fill)
        self.start = GUARD + self.delta
        self.total = self.start + self.size + GUARD
        self.buf = pattern(self.total, fill, device)
        assert self.buf.data_ptr() % 16 == 0, "allocation is not 16-byte aligned"
        self.payload = self.buf[self.start:self.start + self.size]
        self.ptr = self.buf.data_ptr() + self.start

    def set(self, data, offset=0):
        """Copy bytes (numpy / bytes / tensor) into the payload at `offset`."""
        if not isinstance(data, torch.Tensor):
            data = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()
                                    if not isinstance(data, np.ndarray)
                                    else np.ascontiguousarray(data).reshape(-1))
        data = data.reshape(-1)
        assert offset + data.numel() <= self.size
        self.payload[offset:offset + data.numel()].copy_(data)
        return self

    def numpy(self):
        """The payload as a numpy array (a copy for device buffers)."""
        return self.payload.cpu().numpy()

    def changed(self, extents=None):
        """Offsets relative to the payload (front guard negative) of the bytes that must keep
        the pattern and did not: both guards, and with `extents` = [(offset, length), ...] (or a
        boolean numpy mask over the payload, True = writable) every other payload byte."""
        writable = np.zeros(self.total, dtype=bool)
        if extents is None:
            writable[self.start:self.start + self.size] = True
        elif isinstance(extents, np.ndarray):  # a mask over the payload (see strided_mask)
            assert extents.dtype == bool and extents.size == self.size
            writable[self.start:self.start + self.size] = extents
        else:
            for off, ln in extents:
                off, ln = int(off), int(ln)
                assert 0 <= off and off + ln <= self.size, "extent outside the payload"
                writable[self.start + off:self.start + off + ln] = True
        keep = torch.from_numpy(~writable).to(self.buf.device)
        bad = (self.buf != pattern(self.total, self.fill, self.buf.device)) & keep
        return (torch.nonzero(bad).reshape(-1) - self.start).cpu().tolist()

    def assert_guards_intact(self, extents=None, what="buffer"):
        bad = self.changed(extents)
        if bad:
            at = bad[0]
            where = ("front guard" if at < 0 else
                     "back guard" if at >= self.size else "gap between the writable extents")
            raise AssertionError(
                f"{what}: {len(bad)} byte(s) outside the writable extent changed, the first at "
                f"payload offset {at} ({where}; payload {self.size} bytes, delta {self.delta})")


def strided_extents(lines, line_stride, symbols, sym_stride, s, limit=None):
    """Extents of `lines` x `symbols` symbols of s bytes on a (line, symbol) stride grid, cut at
    payload offset `limit` (bytes at or past it are not writable)."""
    out = []
    for line in range(lines):
        for i in range(symbols):
            o = line * line_stride + i * sym_stride
            m = s if limit is None else max(0, min(s, limit - o))
            if m:
                out.append((o, m))
    return out


def strided_mask(size, lines, line_stride, symbols, sym_stride, s, limit=None):
    """strided_extents as a boolean mask over a payload of `size` bytes (True = writable)."""
    o = (np.arange(lines, dtype=np.int64)[:, None, None] * line_stride +
         np.arange(symbols, dtype=np.int64)[None, :, None] * sym_stride +
         np.arange(s, dtype=np.int64)[None, None, :]).reshape(-1)
    if limit is not None:
        o = o[o < limit]
    assert o.size == 0 or o.max() < size, "extent outside the payload"
    mask = np.zeros(size, dtype=bool)
    mask[o] = True
    return mask


_BACKENDS = {}


def ops_backend(name, request):
    """(ops, device) behind the `ops` interface of walrus_amd/partition.py: "cpu" = tests/cpu_ops
    (the numpy oracle on CPU tensors, validates a test body without a GPU), "device" = DeviceOps
    (the HIP engine; needs the `gpu` fixture, which fails loudly without one)."""
    if name not in _BACKENDS:
        if name == "cpu":
            from cpu_ops import CpuOps
            _BACKENDS[name] = (CpuOps(), torch.device("cpu"))
        else:
            request.getfixturevalue("gpu")
            from walrus_amd.partition import DeviceOps
            _BACKENDS[name] = (DeviceOps(), torch.device("cuda", 0))
    return _BACKENDS[name]


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
