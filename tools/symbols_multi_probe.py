#!/usr/bin/env python3
"""Recovery symbols in bulk against the per-request call (the measurement behind DESIGN.md §17).

At n = 1000, s = 1206 (one 256 MiB blob), `--slivers` primary slivers each serve `--targets`
seeded targets, half of them systematic (< k) and half repair.  Paths, alternating, `--reps`
repetitions each after one warm-up of all three, every argument marshalled before the clock starts:
  (a) rs2_verifier_recovery_symbols_device_async with slivers x targets requests, each passing its
      source sliver again (the slivers repeated on the device beforehand)
  (b) one rs2_verifier_recovery_symbols_multi_device_async call, RS2_TREES_BUILD, no d_nodes
  (c) the same call with RS2_TREES_CACHED on trees a BUILD call wrote beforehand
Each repetition is timed from the call to the stream's completion (wall clock, synchronised at
both ends) and its symbols and proofs are compared with path (a)'s; for (b) and (c) the time until
the call returns (host planning and enqueueing) is reported as well, and the
rs2_recovery_symbols_stats counters each path moved.  Exits non-zero when an output differs or
(b) takes more than half of (a).  Prints one JSON line.
usage: python3 tools/symbols_multi_probe.py [--slivers 128] [--targets 10] [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slivers", type=int, default=128)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import walrus_amd as W
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverVerifier, _stream, recovery_symbols_stats
    n, blob_len, M, T = 1000, 256 << 20, args.slivers, args.targets
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    blob = torch.randint(0, 256, (blob_len,), dtype=torch.uint8, device=dev, generator=g)
    plan = W.DevicePlan(n, blob_len)
    info = plan.info
    k, s, pl = info.n_secondary, info.symbol_size, info.primary_sliver_len
    prim = torch.empty(n * pl + 256, dtype=torch.uint8, device=dev)
    sec = torch.empty(n * info.secondary_sliver_len + 256, dtype=torch.uint8, device=dev)
    hashes = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    bid = torch.empty(32, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan.encode_async(blob.data_ptr(), prim.data_ptr(), sec.data_ptr(), hashes.data_ptr(),
                      bid.data_ptr(), st)
    torch.cuda.synchronize()
    del blob, sec, bid
    assert M <= n and pl == k * s
    slivers = prim[:M * pl].clone()                      # primary slivers 0 .. M, back to back
    del prim
    rng = np.random.default_rng(42)
    per = [[int(t) for t in rng.permutation(np.concatenate(
        [rng.integers(0, k, T // 2), rng.integers(k, n, T - T // 2)]))] for _ in range(M)]
    flat = [t for ts in per for t in ts]
    total = M * T
    lib, stp = _lib.lib(), _stream(st)
    L, nn = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.rs2_merkle_tree_shape(n, ctypes.byref(L), ctypes.byref(nn)) == 0
    L, nn = L.value, nn.value
    v = SliverVerifier(n, s, "primary")
    repeated = slivers.view(M, pl).repeat_interleave(T, dim=0).contiguous()   # (a)'s sources
    a_tg = (ctypes.c_uint16 * total)(*flat)
    counts = (ctypes.c_uint32 * M)(*([T] * M))
    sym = torch.zeros(total * s, dtype=torch.uint8, device=dev)
    prf = torch.zeros(total * L * 32, dtype=torch.uint8, device=dev)
    nodes = torch.zeros(M * nn * 32, dtype=torch.uint8, device=dev)
    # the cache of path (c): one BUILD call that hands the trees out
    assert lib.rs2_verifier_recovery_symbols_multi_device_async(
        v.handle, M, slivers.data_ptr(), (ctypes.c_uint32 * M)(), None, _lib.RS2_TREES_BUILD,
        nodes.data_ptr(), None, None, stp) == 0, _lib.last_error()
    torch.cuda.synchronize()
    host_ms = {"b": [], "c": []}

    def path_a():
        return lib.rs2_verifier_recovery_symbols_device_async(
            v.handle, total, repeated.data_ptr(), a_tg, sym.data_ptr(), prf.data_ptr(), None, stp)

    def multi(trees, d_nodes):
        return lib.rs2_verifier_recovery_symbols_multi_device_async(
            v.handle, M, slivers.data_ptr(), counts, a_tg, trees, d_nodes, sym.data_ptr(),
            prf.data_ptr(), stp)

    paths = (("a", path_a), ("b", lambda: multi(_lib.RS2_TREES_BUILD, None)),
             ("c", lambda: multi(_lib.RS2_TREES_CACHED, nodes.data_ptr())))
    want = {}

    def timed(name, fn):
        sym.zero_()
        prf.zero_()
        torch.cuda.synchronize()
        before = recovery_symbols_stats()
        t0 = time.perf_counter()
        rc = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, _lib.last_error()
        after = recovery_symbols_stats()
        if name in host_ms:
            host_ms[name].append(round((t1 - t0) * 1e3, 3))
        if not want:                                     # path (a)'s first run is the reference
            assert name == "a"
            want["sym"], want["prf"] = sym.clone(), prf.clone()
        ok = bool(torch.equal(sym, want["sym"]) and torch.equal(prf, want["prf"]))
        return dt, ok, {key: after[key] - before[key] for key in after}

    ok = True
    for name, fn in paths:
        _, good, _ = timed(name, fn)
        ok = ok and good
    for xs in host_ms.values():
        xs.clear()
    res = {name: [] for name, _ in paths}
    stats = {}
    for _ in range(args.reps):
        for name, fn in paths:
            dt, good, delta = timed(name, fn)
            res[name].append(round(dt, 3))
            stats[name] = delta
            ok = ok and good

    def summary(xs):
        med = sorted(xs)[len(xs) // 2]
        return {"median_ms": med, "min_ms": min(xs), "max_ms": max(xs),
                "spread_ms": round(max(xs) - min(xs), 3), "requests_per_s": round(total / (med / 1e3))}
    a, b, c = (summary(res[key]) for key in "abc")
    ratio = round(b["median_ms"] / a["median_ms"], 4)
    print(json.dumps({
        "n": n, "symbol_size": s, "slivers": M, "targets_per_sliver": T, "requests": total,
        "reps": args.reps, "a_per_request": a, "b_multi_build": b, "c_multi_cached": c,
        "b_host_ms_median": sorted(host_ms["b"])[len(host_ms["b"]) // 2],
        "c_host_ms_median": sorted(host_ms["c"])[len(host_ms["c"]) // 2],
        "b_over_a": ratio, "a_over_b": round(a["median_ms"] / b["median_ms"], 2),
        "a_over_c": round(a["median_ms"] / c["median_ms"], 2),
        "stats_per_call": stats, "ok": ok, "b_within_half_of_a": ratio <= 0.5}), flush=True)
    if not ok or ratio > 0.5:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
