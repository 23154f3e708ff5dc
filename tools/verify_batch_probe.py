#!/usr/bin/env python3
"""Batched decode_and_verify against the per-blob loop (the measurement behind DESIGN.md's
verified-decode-batch section).

`--blobs` blobs of `--blob-mib` MiB at n = 1000 are encoded once (one batch encode) and stay on
the device with their metadata.  Then, per check (Default on the primary axis, and Strict), with a
fresh seeded random K_p subset per blob and repetition:
  (a) a loop of rs2_decode_and_verify_device calls on one plan, one per blob (each returns once
      its verdict is known) -- the path a reader has without the batch call;
  (b) one rs2_decode_and_verify_batch_device_async over all the blobs, then one stream
      synchronize.
(a) and (b) alternate, `--reps` repetitions each after one warm-up of both; every repetition is
timed from the first call to the stream's completion (wall clock, synchronised at both ends) and
checked: every call of (a) returns RS2_OK, (b) leaves `--blobs` MATCH verdicts, and both leave
the blobs.  A separate profiled batch call reports the per-stage times.  Prints one JSON line.
usage: python3 tools/verify_batch_probe.py [--blobs 128] [--reps 3]
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
    args = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import walrus_amd as W
    from walrus_amd import _lib
    from walrus_amd.encoding import _stream, decode_batch_stats, verify_batch_stats
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
    del sec
    # the per-blob call takes host copies of the metadata
    h_hashes = hashes.cpu().numpy()
    h_ids = ids.cpu().numpy()
    K, L = info.n_primary, pl
    out = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
    verdict = torch.zeros(B, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(42)
    lib, h, stp = _lib.lib(), plan.handle, _stream(st)
    out_ptrs = [out[b].data_ptr() for b in range(B)]
    u16p, u64p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint64)
    counts = (ctypes.c_uint32 * B)(*([K] * B))

    # arguments are marshalled before the clock starts, as in tools/dec_batch_probe.py
    def fresh():
        subs = [rng.permutation(n)[:K] for _ in range(B)]
        idx = np.concatenate(subs).astype(np.uint16)
        off = np.concatenate([(np.uint64(b * n) + sel.astype(np.uint64)) * np.uint64(L)
                              for b, sel in enumerate(subs)]).astype(np.uint64)
        return idx, off

    def loop(items, check):
        idx, off = items
        for b in range(B):
            rc = lib.rs2_decode_and_verify_device(
                h, 0, K, ctypes.cast(idx.ctypes.data + 2 * b * K, u16p), prim.data_ptr(),
                ctypes.cast(off.ctypes.data + 8 * b * K, u64p),
                h_hashes.ctypes.data + b * n * 64, h_ids.ctypes.data + b * 32, check,
                out_ptrs[b], stp)
            assert rc == 0, _lib.last_error()
        return True

    def batch(items, check):
        idx, off = items
        rc = lib.rs2_decode_and_verify_batch_device_async(
            h, 0, B, None, counts, idx.ctypes.data_as(u16p), prim.data_ptr(),
            off.ctypes.data_as(u64p), hashes.data_ptr(), ids.data_ptr(), check, out.data_ptr(),
            stride, verdict.data_ptr(), None, stp)
        assert rc == 0, _lib.last_error()
        torch.cuda.current_stream(dev).synchronize()
        return bool((verdict == _lib.RS2_BLOB_MATCH).all())

    def timed(fn, check):
        items = fresh()
        out.zero_()
        verdict.fill_(-1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        good = fn(items, check)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        return dt, good and bool(torch.equal(out[:, :blob_len], blobs[:, :blob_len]))

    def summary(xs):
        return {"ms": xs, "median_ms": sorted(xs)[len(xs) // 2],
                "spread_ms": round(max(xs) - min(xs), 3)}

    report = {"n": n, "blobs": B, "blob_bytes": blob_len, "symbol_size": info.symbol_size}
    gib = B * blob_len / 2 ** 30
    for name, check in (("default", _lib.CHECK_DEFAULT), ("strict", _lib.CHECK_STRICT)):
        ok = timed(loop, check)[1] and timed(batch, check)[1]
        before, dbefore = verify_batch_stats(), decode_batch_stats()
        res = {"loop": [], "batch": []}
        for _ in range(args.reps):
            for kind, fn in (("loop", loop), ("batch", batch)):
                dt, good = timed(fn, check)
                res[kind].append(round(dt, 3))
                ok = ok and good
        after, dafter = verify_batch_stats(), decode_batch_stats()
        plan.profile(True)
        ok = timed(batch, check)[1] and ok
        prof = {k: [round(v[0], 3), v[1]] for k, v in plan.profile_read().items()}
        plan.profile(False)
        loop_s, batch_s = summary(res["loop"]), summary(res["batch"])
        report[name] = {
            "loop": loop_s, "batch": batch_s,
            "loop_gib_s": round(gib / (loop_s["median_ms"] / 1e3), 2),
            "batch_gib_s": round(gib / (batch_s["median_ms"] / 1e3), 2),
            "speedup": round(loop_s["median_ms"] / batch_s["median_ms"], 2),
            "verify_stats_delta": {k: after[k] - before[k] for k in after},
            "decode_stats_delta": {k: dafter[k] - dbefore[k] for k in dafter},
            "profile_one_batch_call": prof, "ok": ok}
    print(json.dumps(report))
    return 0 if all(report[k]["ok"] for k in ("default", "strict")) else 1


if __name__ == "__main__":
    sys.exit(main())
