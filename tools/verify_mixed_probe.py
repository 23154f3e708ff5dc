#!/usr/bin/env python3
"""Mixed sliver verification against the per-size loop (the measurement behind DESIGN.md §19).

At n = 1000 on the primary axis, `--slivers` (128) seeded random slivers, every argument marshalled
before the clock starts, each repetition timed from the call to the stream's completion (wall
clock, synchronised at both ends), paths alternating, one warm-up of each, `--reps` repetitions:
 (1) mixed: 64 distinct even symbol sizes spread over 4 .. 300, two slivers each
     (a) a loop of rs2_verifier_roots_device_async over verifiers created beforehand, one per size
     (b) one rs2_sliver_checker_verify_device_async call (also: the time until it returns)
 (2) uniform: every sliver at s = 1206
     (a') one rs2_verifier_roots_device_async call
     (b)  one rs2_sliver_checker_verify_device_async call
Roots are compared bit for bit.  Exits non-zero when a root differs or (1b) is not faster than
(1a); (2) has no pass mark, its ratio says which call a uniform batch should use.  Prints one JSON
line.
usage: python3 tools/verify_mixed_probe.py [--slivers 128] [--reps 20]
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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverChecker, SliverVerifier, _stream, verify_mixed_stats
    n, M = 1000, args.slivers
    k = n - (n - 1) // 3                                  # K_s: symbols of a primary sliver
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    stp = _stream(st)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    checker = SliverChecker(n)

    def setup(sizes):
        """Slivers of `sizes` (one per sliver) back to back; the per-size runs of path (a)."""
        off, at = [], 0
        for s in sizes:
            off.append(at)
            at += k * s
        data = torch.randint(0, 256, (at,), dtype=torch.uint8, device=dev, generator=g)
        runs = []                                         # (verifier, count, first sliver)
        for i, s in enumerate(sizes):
            if runs and sizes[i - 1] == s:
                runs[-1][1] += 1
            else:
                runs.append([SliverVerifier(n, s, "primary"), 1, i])
        m = len(sizes)
        return {"m": m, "data": data, "off": off, "runs": runs,
                "axes": (ctypes.c_uint8 * m)(), "sizes": (ctypes.c_uint16 * m)(*sizes),
                "offs": (ctypes.c_uint64 * m)(*off),
                "roots": torch.zeros(m * 32, dtype=torch.uint8, device=dev)}

    def loop(c):
        base, roots = c["data"].data_ptr(), c["roots"].data_ptr()
        for v, count, first in c["runs"]:
            rc = lib.rs2_verifier_roots_device_async(v.handle, count, base + c["off"][first],
                                                     roots + 32 * first, stp)
            if rc:
                return rc
        return 0

    def mixed(c):
        return lib.rs2_sliver_checker_verify_device_async(
            checker.handle, c["m"], c["axes"], c["sizes"], c["data"].data_ptr(), c["offs"], None,
            c["roots"].data_ptr(), None, None, stp)

    def timed(c, fn):
        c["roots"].zero_()
        torch.cuda.synchronize()
        before = verify_mixed_stats()
        t0 = time.perf_counter()
        rc = fn(c)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, _lib.last_error()
        after = verify_mixed_stats()
        return dt, (t1 - t0) * 1e3, c["roots"].clone(), {x: after[x] - before[x] for x in after}

    def summary(xs):
        med = sorted(xs)[len(xs) // 2]
        return {"median_ms": round(med, 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
                "spread_ms": round(max(xs) - min(xs), 3)}

    def compare(c):
        _, _, want, _ = timed(c, loop)                    # warm-up of each; (a) is the reference
        _, _, got, _ = timed(c, mixed)
        ok = bool(torch.equal(want, got))
        res = {"a": [], "b": []}
        host, stats = [], {}
        for _ in range(args.reps):
            dt, _, r, _ = timed(c, loop)
            res["a"].append(dt)
            ok = ok and bool(torch.equal(r, want))
            dt, h, r, stats = timed(c, mixed)
            res["b"].append(dt)
            host.append(h)
            ok = ok and bool(torch.equal(r, want))
        a, b = summary(res["a"]), summary(res["b"])
        return {"a_per_size": a, "b_mixed": b,
                "b_host_ms_median": round(sorted(host)[len(host) // 2], 3),
                "a_over_b": round(a["median_ms"] / b["median_ms"], 2),
                "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
                "per_size_calls": len(c["runs"]), "stats_per_call": stats, "ok": ok}

    distinct = [4 + 2 * ((i * 148) // 63) for i in range(64)]   # 64 even sizes over 4 .. 300
    assert len(set(distinct)) == 64 and min(distinct) == 4 and max(distinct) == 300
    per = max(1, M // 64)
    mix = compare(setup([s for s in distinct for _ in range(per)]))
    uni = compare(setup([1206] * M))
    faster = mix["b_mixed"]["median_ms"] < mix["a_per_size"]["median_ms"]
    ok = mix["ok"] and uni["ok"]
    print(json.dumps({"n": n, "axis": "primary", "slivers": M, "reps": args.reps,
                      "mixed_64_sizes": mix, "uniform_s1206": uni, "ok": ok,
                      "mixed_b_faster_than_a": faster}), flush=True)
    if not ok or not faster:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
