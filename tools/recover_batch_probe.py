#!/usr/bin/env python3
"""Batched sliver recovery against the per-sliver paths (the measurement behind DESIGN.md §15).

At n = 1000, `--slivers` primary slivers are recovered, each from a fresh seeded random K_s subset
of its recovery symbols, gathered on the device from the encoded secondary slivers:
  big    s = 1206: the slivers of one 256 MiB blob
  small  s = 20:   the slivers of 4 MiB blobs
Paths, alternating, `--reps` repetitions each after one warm-up of all three, every argument
marshalled before the clock starts, every repetition checked against the encoded slivers and the
metadata hashes:
  (a) host: rs2_decode_1d then rs2_sliver_merkle_root per sliver (host buffers in and out)
  (b) device loop: rs2_codec_decode_device_async with lines = 1, then
      rs2_verifier_roots_device_async with count = 1, per sliver
  (c) one rs2_verifier_recover_slivers_device_async call
Each repetition is timed from the first call to the stream's completion (wall clock, synchronised
at both ends); for (c) the time until the call returns (host planning and enqueueing) is reported
as well.  Prints one JSON line per shape.
usage: python3 tools/recover_batch_probe.py [--slivers 128] [--reps 3] [--shapes big,small]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_shape(shape, blob_len, n_blobs, M, reps):
    import numpy as np
    import torch
    import walrus_amd as W
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverVerifier, _stream, recover_stats
    n = 1000
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    stride = (blob_len + 255) // 256 * 256
    blobs = torch.randint(0, 256, (n_blobs, stride), dtype=torch.uint8, device=dev, generator=g)
    plan = W.DevicePlan(n, blob_len)
    info = plan.info
    kp, ks, s = info.n_primary, info.n_secondary, info.symbol_size
    pl, sl = info.primary_sliver_len, info.secondary_sliver_len
    prim = torch.empty((n_blobs, n * pl), dtype=torch.uint8, device=dev)
    sec = torch.empty((n_blobs, n * sl), dtype=torch.uint8, device=dev)
    hashes = torch.empty(n_blobs * n * 64, dtype=torch.uint8, device=dev)
    ids = torch.empty(n_blobs * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan.encode_batch_async(n_blobs, blobs.data_ptr(), stride, None, prim.data_ptr(), n * pl,
                            sec.data_ptr(), n * sl, hashes.data_ptr(), ids.data_ptr(), st)
    torch.cuda.synchronize()
    del blobs, ids
    K = ks  # a primary sliver has K_s symbols and is recovered from K_s of its n recovery symbols
    per_blob = M // n_blobs
    targets = [(b, t) for b in range(n_blobs) for t in range(per_blob)]  # t < K_p
    assert per_blob <= kp and len(targets) == M
    want = torch.stack([prim[b].view(n, pl)[t] for b, t in targets])          # (M, K*s)
    want_roots = torch.stack([hashes.view(n_blobs, n, 64)[b, t, :32] for b, t in targets])
    expected = want_roots.cpu().numpy().tobytes()
    secv = sec.view(n_blobs, n, kp, s)
    rng = np.random.default_rng(42)
    lib, stp = _lib.lib(), _stream(st)
    v = SliverVerifier(n, s, "primary")
    codec = ctypes.c_void_p()
    assert lib.rs2_codec_create(K, n, s, ctypes.byref(codec)) == 0, _lib.last_error()
    out = torch.zeros((M, K * s), dtype=torch.uint8, device=dev)
    roots = torch.zeros((M, 32), dtype=torch.uint8, device=dev)
    verdict = torch.zeros(M, dtype=torch.int32, device=dev)
    exp_c = (ctypes.c_uint8 * len(expected)).from_buffer_copy(expected)
    counts = (ctypes.c_uint32 * M)(*([K] * M))
    u16p, u64p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint64)
    sym_off = (np.arange(K, dtype=np.uint64) * np.uint64(s))
    out_h = np.zeros((M, K * s), dtype=np.uint8)
    roots_h = np.zeros((M, 32), dtype=np.uint8)

    def fresh(host):
        """A K-subset of the n recovery symbols per sliver; the symbols back to back on the
        device (and, for the host path, on the host with one pointer per symbol)."""
        subs = [rng.permutation(n)[:K] for _ in range(M)]
        idx = np.concatenate(subs).astype(np.uint16)
        syms = torch.empty((M, K, s), dtype=torch.uint8, device=dev)
        for i, ((b, t), sel) in enumerate(zip(targets, subs)):
            syms[i] = secv[b, torch.from_numpy(sel.astype(np.int64)).to(dev), t]
        item = {"idx": idx, "syms": syms}
        if host:
            h = syms.cpu().numpy()
            base = h.ctypes.data
            item["host"] = h
            item["ptrs"] = (ctypes.c_void_p * (M * K))(*[base + j * s for j in range(M * K)])
        return item

    def path_a(it):
        idx, ptrs = it["idx"], it["ptrs"]
        for i in range(M):
            rc = lib.rs2_decode_1d(K, n, s, K, ctypes.cast(idx.ctypes.data + 2 * i * K, u16p),
                                   ctypes.cast(ctypes.addressof(ptrs) + 8 * i * K,
                                               ctypes.POINTER(ctypes.c_void_p)),
                                   out_h[i].ctypes.data)
            assert rc == 0, _lib.last_error()
            rc = lib.rs2_sliver_merkle_root(n, s, 0, out_h[i].ctypes.data, K * s,
                                            roots_h[i].ctypes.data)
            assert rc == 0, _lib.last_error()

    def path_b(it):
        idx, syms = it["idx"], it["syms"]
        off = sym_off.ctypes.data_as(u64p)
        for i in range(M):
            rc = lib.rs2_codec_decode_device_async(
                codec, 1, K, ctypes.cast(idx.ctypes.data + 2 * i * K, u16p), syms[i].data_ptr(),
                off, 0, out[i].data_ptr(), s, 0, K * s, stp)
            assert rc == 0, _lib.last_error()
            rc = lib.rs2_verifier_roots_device_async(v.handle, 1, out[i].data_ptr(),
                                                     roots[i].data_ptr(), stp)
            assert rc == 0, _lib.last_error()

    host_ms = []

    def path_c(it):
        idx, syms = it["idx"], it["syms"]
        t0 = time.perf_counter()
        rc = lib.rs2_verifier_recover_slivers_device_async(
            v.handle, M, counts, idx.ctypes.data_as(u16p), syms.data_ptr(), exp_c, out.data_ptr(),
            roots.data_ptr(), verdict.data_ptr(), None, stp)
        host_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        assert rc == 0, _lib.last_error()

    def timed(name, fn):
        it = fresh(host=name == "a")
        out.zero_()
        roots.zero_()
        verdict.zero_()
        out_h[:] = 0
        roots_h[:] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(it)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if name == "a":
            ok = bool(np.array_equal(out_h, want.cpu().numpy()) and
                      np.array_equal(roots_h, want_roots.cpu().numpy()))
        else:
            ok = bool(torch.equal(out, want) and torch.equal(roots, want_roots))
            if name == "c":
                ok = ok and bool((verdict == 1).all())
        return dt, ok

    paths = (("a", path_a), ("b", path_b), ("c", path_c))
    for name, fn in paths:
        timed(name, fn)
    host_ms.clear()
    before = recover_stats()
    res = {name: [] for name, _ in paths}
    ok = True
    for _ in range(reps):
        for name, fn in paths:
            dt, good = timed(name, fn)
            res[name].append(round(dt, 3))
            ok = ok and good
    after = recover_stats()
    # one more (c) call with the verifier's stage profiler on: host planning, setup, kernels
    v.profile(True)
    _, good = timed("c", path_c)
    ok = ok and good
    prof = {k: [round(t, 3), c] for k, (t, c) in v.profile_read().items()}
    v.profile(False)
    host_ms.pop()
    lib.rs2_codec_destroy(codec)

    def summary(xs):
        med = sorted(xs)[len(xs) // 2]
        return {"ms": xs, "median_ms": med, "spread_ms": round(max(xs) - min(xs), 3),
                "slivers_per_s": round(M / (med / 1e3))}
    a, b, c = (summary(res[k]) for k in "abc")
    print(json.dumps({
        "shape": shape, "n": n, "symbol_size": s, "slivers": M, "symbols_per_sliver": K,
        "a_host_per_sliver": a, "b_device_loop": b, "c_one_call": c,
        "c_host_ms": host_ms, "b_over_c": round(b["median_ms"] / c["median_ms"], 2),
        "a_over_c": round(a["median_ms"] / c["median_ms"], 2),
        "recover_stats_delta": {k: after[k] - before[k] for k in after},
        "profile_one_c_call": prof, "ok": ok}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slivers", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="big,small")
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        if shape == "big":
            run_shape("big", 256 << 20, 1, args.slivers, args.reps)
        elif shape == "small":
            run_shape("small", 4 << 20, 4, args.slivers, args.reps)
        else:
            raise SystemExit(f"unknown shape {shape}")


if __name__ == "__main__":
    main()
