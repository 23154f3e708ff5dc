#!/usr/bin/env python3
"""Batched decode against the per-blob loop (the measurement behind DESIGN.md's decode-batch
section).

`--blobs` blobs of `--blob-mib` MiB at n = 1000 are encoded once (one batch encode) and stay on
the device.  Then, with a fresh seeded random K_p subset per blob and repetition:
  (a) a loop of rs2_decode_device_async calls on one plan, one per blob -- the path a caller
      has without the batch call;
  (b) one rs2_decode_batch_device_async over all the blobs.
(a) and (b) alternate, `--reps` repetitions each after one warm-up of both; every repetition is
timed from the first call to the stream's completion (wall clock, synchronised at both ends).
A separate profiled batch call reports the host planning time and the per-stage device times.
Prints one JSON line.  usage: python3 tools/dec_batch_probe.py [--blobs 128] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=128)
    ap.add_argument("--blob-mib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--axis", default="primary", choices=["primary", "secondary"])
    args = ap.parse_args()
    import numpy as np
    import torch
    import walrus_amd as W
    from walrus_amd.encoding import decode_batch_stats
    n, B = 1000, args.blobs
    blob_len = int(args.blob_mib * (1 << 20))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    stride = (blob_len + 255) // 256 * 256
    blobs = torch.randint(0, 256, (B, stride), dtype=torch.uint8, device=dev, generator=g)
    plan = W.DevicePlan(n, blob_len)
    info = plan.info
    pl, sl = info.primary_sliver_len, info.secondary_sliver_len
    prim = torch.empty((B, n * pl), dtype=torch.uint8, device=dev)
    sec = torch.empty((B, n * sl), dtype=torch.uint8, device=dev)
    hashes = torch.empty(B * n * 64, dtype=torch.uint8, device=dev)
    ids = torch.empty(B * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan.encode_batch_async(B, blobs.data_ptr(), stride, None, prim.data_ptr(), n * pl,
                            sec.data_ptr(), n * sl, hashes.data_ptr(), ids.data_ptr(), st)
    torch.cuda.synchronize()
    del hashes, ids
    src, L, K = (prim, pl, info.n_primary) if args.axis == "primary" else (sec, sl, info.n_secondary)
    out = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(42)

    # Both paths are called through the C ABI with their arguments marshalled before the clock
    # starts (a Python list of 128 x 334 indices takes longer to turn into a C array than either
    # path takes to run), so the times are the engine's: its host work plus the device work.
    import ctypes
    from walrus_amd import _lib
    lib, h, ax = _lib.lib(), plan.handle, 0 if args.axis == "primary" else 1
    from walrus_amd.encoding import _stream
    stp = _stream(st)
    out_ptrs = [out[b].data_ptr() for b in range(B)]

    def fresh():
        subs = [rng.permutation(n)[:K] for _ in range(B)]
        idx = np.concatenate(subs).astype(np.uint16)
        off = np.concatenate([(np.uint64(b * n) + sel.astype(np.uint64)) * np.uint64(L)
                              for b, sel in enumerate(subs)]).astype(np.uint64)
        return (idx, off, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))

    counts = (ctypes.c_uint32 * B)(*([K] * B))
    u16p, u64p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint64)

    def loop(items):
        idx, off, _, _ = items
        for b in range(B):
            rc = lib.rs2_decode_device_async(
                h, ax, K, ctypes.cast(idx.ctypes.data + 2 * b * K, u16p), src.data_ptr(),
                ctypes.cast(off.ctypes.data + 8 * b * K, u64p), out_ptrs[b], stp)
            assert rc == 0, _lib.last_error()

    def batch(items):
        _, _, pi, po = items
        rc = lib.rs2_decode_batch_device_async(h, ax, B, None, counts, pi, src.data_ptr(), po,
                                               out.data_ptr(), stride, None, stp)
        assert rc == 0, _lib.last_error()

    def timed(fn):
        items = fresh()
        out.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(items)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        ok = bool(torch.equal(out[:, :blob_len], blobs[:, :blob_len]))
        return dt, ok

    timed(loop)
    timed(batch)
    before = decode_batch_stats()
    res = {"loop": [], "batch": []}
    ok = True
    for _ in range(args.reps):
        for name, fn in (("loop", loop), ("batch", batch)):
            dt, good = timed(fn)
            res[name].append(round(dt, 3))
            ok = ok and good
    after = decode_batch_stats()
    plan.profile(True)
    timed(batch)
    prof = {k: [round(v[0], 3), v[1]] for k, v in plan.profile_read().items()}
    plan.profile(False)

    def summary(xs):
        return {"ms": xs, "median_ms": sorted(xs)[len(xs) // 2], "spread_ms": round(max(xs) - min(xs), 3)}
    gib = B * blob_len / 2 ** 30
    loop_s, batch_s = summary(res["loop"]), summary(res["batch"])
    print(json.dumps({
        "n": n, "blobs": B, "blob_bytes": blob_len, "axis": args.axis, "symbol_size": info.symbol_size,
        "loop": loop_s, "batch": batch_s,
        "loop_gib_s": round(gib / (loop_s["median_ms"] / 1e3), 2),
        "batch_gib_s": round(gib / (batch_s["median_ms"] / 1e3), 2),
        "speedup": round(loop_s["median_ms"] / batch_s["median_ms"], 2),
        "batch_stats_delta": {k: after[k] - before[k] for k in after},
        "profile_one_batch_call": prof, "ok": ok}))


if __name__ == "__main__":
    main()
