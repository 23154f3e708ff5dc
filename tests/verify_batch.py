"""Shared body of the verified-decode-batch tests -- TEST ONLY (a plain module: no fixtures; torch
is imported by the functions that need a device).

One batched call holds many corruption cases (tests/corruption.py) of one geometry, axis and
check side by side: blob b is case b, decoded from its own slivers and checked against its own
metadata, so honest and corrupted blobs share a launch.  The model decides every verdict and, on
a match, every byte.

  batch_cases(gid, axis, check)   the cases of one call: every layout of the axis, both
                                  scenarios, zero-length blobs left out, the layout's honest
                                  case after every fourth case
  pack(cases)                     what the call passes, as host arrays
  DeviceCall                      the device buffers of one call shape and run(packed, ...)
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import corruption as C

MISMATCH, MATCH, SKIPPED = 0, 1, 2
OUT_FILL = 0xEE
VERDICT_FILL = 0x5A5A5A5A


def batch_cases(gid: str, axis: str, check: str, honest_every: int = 4) -> list:
    g = C.GEOMETRIES[gid]
    lay = C.layouts(gid)
    out = []
    own = [c for c in C.cases(gid)
           if c.check == check and lay[c.layout][0] == axis and g.length + c.dlen != 0]
    for i, c in enumerate(own):
        out.append(c)
        if (i + 1) % honest_every == 0:
            out.append(c.honest())
    return out


def pulled(idx, need: int) -> int:
    """select_slivers restated: input items consumed, the one that finds the workspace full
    included."""
    chosen = set()
    for i, q in enumerate(idx):
        if len(chosen) == need:
            return i + 1
        chosen.add(q)
    return len(idx)


def model_rows(p, axis: str, idx, length: int) -> list:
    """corruption.model_verify's rule: [(row, its bytes inside the blob)] of the rows the Default
    check hashes for slivers `idx` (input order) of `axis`."""
    verified = set()
    if axis == C.PRIMARY:
        taken = set()
        for i in idx:
            if i < p.n_primary:
                verified.add(i)
            if len(taken) == p.n_primary:
                break
            taken.add(i)
    row = p.n_secondary * p.symbol_size
    return [(i, min(row, max(0, length - i * row))) for i in range(p.n_primary)
            if i not in verified]


def default_need(p, rows: int) -> int:
    """Check scratch of a blob under Default (include/walrus_rs2.h, the window budget): per row
    the gathered row, its n leaves and its repair symbols."""
    n, ks, s = p.n_shards, p.n_secondary, p.symbol_size
    return rows * (ks * s + n * 32 + (n - ks) * s)


def strict_need(p) -> int:
    """Check scratch of a blob under Strict: its slivers, repair quadrant and leaves."""
    n, kp, ks, s = p.n_shards, p.n_primary, p.n_secondary, p.symbol_size
    return n * (ks * s + kp * s) + (n - kp) * (n - ks) * s + n * n * 32


def windows(need, budget: int, max_blobs: int = 341) -> int:
    """The window rule restated: the number of windows over the slots' needs."""
    count, used, held = 0, 0, 0
    for v in need:
        if held and (held == max_blobs or used + v > budget):
            count, used, held = count + 1, 0, 0
        used += v
        held += 1
    return count + (1 if held else 0)


def model_verdicts(cases) -> list:
    """[("ok", bytes) | ("rejected",)] per case."""
    return [C.expected(c) for c in cases]


@dataclass
class Packed:
    n: int
    axis: str
    slivers: np.ndarray          # every blob's slivers back to back, blob after blob
    blobs: list                  # [(indices, offsets from the sliver base)]
    lens: List[int]
    hashes: np.ndarray           # B * 64 n
    ids: np.ndarray              # B * 32
    sliver_len: int


def pack(cases, honest: bool = False) -> Packed:
    """honest=True: every case replaced by its layout's honest case (same shape)."""
    parts, blobs, lens, hashes, ids = [], [], [], [], []
    at = 0
    n = axis = ln = None
    for c in cases:
        m = C.materialise(c.honest() if honest else c)
        n, axis = m["n"], m["axis"]
        idx, offs = [], []
        for i, d in m["slivers"]:
            ln = len(d)
            idx.append(i)
            offs.append(at)
            parts.append(np.frombuffer(d, np.uint8))
            at += ln
        blobs.append((idx, offs))
        lens.append(m["length"])
        hashes.append(b"".join(p + q for p, q in m["hashes"]))
        ids.append(m["blob_id"])
    return Packed(n, axis, np.concatenate(parts), blobs, lens,
                  np.frombuffer(b"".join(hashes), np.uint8).copy(),
                  np.frombuffer(b"".join(ids), np.uint8).copy(), ln)


class DeviceCall:
    """Device buffers for calls of one shape (B blobs, a sliver buffer size) on one DevicePlan;
    the addresses stay the same from run to run."""

    def __init__(self, gpu, plan, packed: Packed, out_stride: Optional[int] = None):
        import torch
        self.torch = torch
        self.gpu = gpu
        self.plan = plan
        dev = torch.device("cuda", 0)
        B = len(packed.blobs)
        self.B = B
        top = max(packed.lens)
        self.out_stride = out_stride if out_stride is not None else (top + 37) // 2 * 2
        self.slivers = torch.zeros(packed.slivers.size, dtype=torch.uint8, device=dev)
        self.hashes = torch.zeros(packed.hashes.size, dtype=torch.uint8, device=dev)
        self.ids = torch.zeros(packed.ids.size, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(B * self.out_stride, dtype=torch.uint8, device=dev)
        self.verdict = torch.zeros(B, dtype=torch.int32, device=dev)

    def run(self, packed: Packed, check: str, stream=None, statuses=False, blobs=None,
            lens=None):
        """Upload, prefill, call, read back: (verdicts, out bytes as (B, out_stride), statuses)."""
        torch = self.torch
        self.slivers.copy_(torch.from_numpy(packed.slivers))
        self.hashes.copy_(torch.from_numpy(packed.hashes))
        self.ids.copy_(torch.from_numpy(packed.ids))
        self.out.fill_(OUT_FILL)
        self.verdict.fill_(VERDICT_FILL)
        torch.cuda.synchronize()
        st = self.plan.decode_and_verify_batch_async(
            packed.axis, blobs if blobs is not None else packed.blobs, self.slivers.data_ptr(),
            self.out.data_ptr(), self.out_stride, self.hashes.data_ptr(), self.ids.data_ptr(),
            check, self.verdict.data_ptr(), blob_lens=lens if lens is not None else packed.lens,
            stream=stream, statuses=statuses)
        self.plan.sync(stream)
        torch.cuda.synchronize()
        return (self.verdict.cpu().numpy().copy(),
                self.out.cpu().numpy().reshape(self.B, self.out_stride).copy(), st)


def raw_call(plan, axis, blobs, lens, d_base, d_hashes, d_ids, check, d_out, out_stride,
             d_verdict, statuses=False, stream=None, n_blobs=None):
    """rs2_decode_and_verify_batch_device_async as the C caller sees it: (return code, status
    list or None).  `check` is the ABI's integer; pointers are integers (0 = NULL)."""
    import ctypes
    from walrus_amd import _lib
    B = len(blobs) if n_blobs is None else n_blobs
    m = max(len(blobs), 1)
    counts = (ctypes.c_uint32 * m)(*[len(ix) for ix, _ in blobs])
    idx = np.concatenate([np.asarray(ix, dtype=np.uint16) for ix, _ in blobs] +
                         [np.zeros(1, dtype=np.uint16)])
    off = np.concatenate([np.asarray(of, dtype=np.uint64) for _, of in blobs] +
                         [np.zeros(1, dtype=np.uint64)])
    cl = (ctypes.c_uint64 * m)(*lens) if lens is not None else None
    status = (ctypes.c_int * m)() if statuses else None
    rc = _lib.lib().rs2_decode_and_verify_batch_device_async(
        plan.handle, int(axis == C.SECONDARY), B, cl, counts,
        idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), d_base,
        off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), d_hashes or None, d_ids or None,
        check, d_out, out_stride, d_verdict or None, status, stream)
    return rc, ([int(v) for v in status[:B]] if statuses else None)


def assert_against_model(cases, want, verdicts, out, lens, what=""):
    """Verdict b equals the model's; on a match the slot holds the model's bytes; every byte at
    or past each blob's length (the stride padding included) keeps its prefill."""
    for b, (c, w) in enumerate(zip(cases, want)):
        v = MATCH if w[0] == "ok" else MISMATCH
        assert verdicts[b] == v, f"{what} blob {b}: verdict {verdicts[b]}, the model says {w[0]}: " \
                                 f"{c.describe()}"
        if v == MATCH:
            assert out[b, :lens[b]].tobytes() == w[1], f"{what} blob {b}: {c.describe()}"
        assert (out[b, lens[b]:] == OUT_FILL).all(), \
            f"{what} blob {b} wrote at or past its length: {c.describe()}"
