#!/usr/bin/env python3
"""Mixed blob encode against the per-size loop (the measurement behind DESIGN.md §22).

At n = 1000, device-resident seeded random blobs, every argument marshalled before the clock
starts, each repetition timed from the call to the stream's completion (wall clock, synchronised at
both ends), paths alternating, one warm-up of each, `--reps` repetitions:
 (1) mixed: 32 distinct even symbol sizes 4 .. 66, two blobs each
     (a) a loop of rs2_encode_batch_device_async over plans created beforehand, one per size
     (b) one rs2_blob_encoder_encode_device_async call (also: the time until it returns)
 (2) uniform: 64 blobs at s = 20
     (a') one rs2_encode_batch_device_async call
     (b)  one rs2_blob_encoder_encode_device_async call
Slivers, pair hashes and ids are compared bit for bit.  Exits non-zero when a byte differs or the
median of (1b) is not below the fastest repetition of (1a); (2) has no pass mark, its ratio says
which call a uniform batch should use.  Prints one JSON line.
usage: python3 tools/encode_mixed_probe.py [--reps 20]
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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from walrus_amd import _lib
    from walrus_amd.encoding import BlobEncoder, DevicePlan, _stream, encode_mixed_stats
    n = 1000
    f = (n - 1) // 3
    kp, ks = n - 2 * f, n - f
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    stp = _stream(st)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    encoder = BlobEncoder(n)

    def setup(sizes):
        """Blobs of `sizes` (one per blob, equal sizes neighbours), each 7 bytes short of its
        message; the per-size runs of path (a)."""
        lens = [s * kp * ks - 7 for s in sizes]
        boff, poff, soff, at, pat, sat = [], [], [], 0, 0, 0
        for s in sizes:
            boff.append(at)
            poff.append(pat)
            soff.append(sat)
            at += s * kp * ks               # the stride of a size's blobs in path (a)
            pat += n * ks * s
            sat += n * kp * s
        m = len(sizes)
        data = torch.randint(0, 256, (at,), dtype=torch.uint8, device=dev, generator=g)
        runs = []                           # [plan, count, first blob, lens array]
        for i, s in enumerate(sizes):
            if runs and sizes[i - 1] == s:
                runs[-1][1] += 1
            else:
                runs.append([DevicePlan(n, lens[i]), 1, i, None])
        for r in runs:
            r[3] = (ctypes.c_uint64 * r[1])(*lens[r[2]:r[2] + r[1]])
        u64 = lambda v: (ctypes.c_uint64 * m)(*v)  # noqa: E731
        z = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)  # noqa: E731
        return {"m": m, "sizes": sizes, "data": data, "boff": boff, "poff": poff, "soff": soff,
                "runs": runs, "a_lens": u64(lens), "a_boff": u64(boff), "a_poff": u64(poff),
                "a_soff": u64(soff), "out": [z(pat), z(sat), z(m * n * 64), z(m * 32)]}

    def loop(c):
        base = c["data"].data_ptr()
        prim, sec, hashes, ids = (t.data_ptr() for t in c["out"])
        for plan, count, first, lens in c["runs"]:
            s = c["sizes"][first]
            rc = lib.rs2_encode_batch_device_async(
                plan.handle, count, base + c["boff"][first], s * kp * ks, lens,
                prim + c["poff"][first], n * ks * s, sec + c["soff"][first], n * kp * s,
                hashes + first * n * 64, ids + first * 32, stp)
            if rc:
                return rc
        return 0

    def mixed(c):
        prim, sec, hashes, ids = (t.data_ptr() for t in c["out"])
        return lib.rs2_blob_encoder_encode_device_async(
            encoder.handle, c["m"], c["a_lens"], c["data"].data_ptr(), c["a_boff"], prim,
            c["a_poff"], sec, c["a_soff"], hashes, ids, None, stp)

    def timed(c, fn):
        for t in c["out"]:
            t.zero_()
        torch.cuda.synchronize()
        before = encode_mixed_stats()
        t0 = time.perf_counter()
        rc = fn(c)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, _lib.last_error()
        after = encode_mixed_stats()
        return dt, (t1 - t0) * 1e3, {x: after[x] - before[x] for x in after}

    def same(c, want):
        return all(bool(torch.equal(a, b)) for a, b in zip(c["out"], want))

    def summary(xs):
        med = sorted(xs)[len(xs) // 2]
        return {"median_ms": round(med, 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
                "spread_ms": round(max(xs) - min(xs), 3)}

    def compare(c):
        timed(c, loop)                                    # warm-up of each; (a) is the reference
        want = [t.clone() for t in c["out"]]
        timed(c, mixed)
        ok = same(c, want)
        res = {"a": [], "b": []}
        host, stats = [], {}
        for _ in range(args.reps):
            dt, _, _ = timed(c, loop)
            res["a"].append(dt)
            ok = ok and same(c, want)
            dt, h, stats = timed(c, mixed)
            res["b"].append(dt)
            host.append(h)
            ok = ok and same(c, want)
        a, b = summary(res["a"]), summary(res["b"])
        return {"a_per_size": a, "b_mixed": b,
                "b_host_ms_median": round(sorted(host)[len(host) // 2], 3),
                "a_over_b": round(a["median_ms"] / b["median_ms"], 2),
                "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
                "per_size_calls": len(c["runs"]), "stats_per_call": stats, "ok": ok}

    distinct = list(range(4, 68, 2))                      # 32 even sizes 4 .. 66
    assert len(distinct) == 32
    mix = compare(setup([s for s in distinct for _ in range(2)]))
    uni = compare(setup([20] * 64))
    faster = mix["b_mixed"]["median_ms"] < mix["a_per_size"]["min_ms"]
    ok = mix["ok"] and uni["ok"]
    print(json.dumps({"n": n, "reps": args.reps, "mixed_32_sizes": mix, "uniform_s20": uni,
                      "ok": ok, "mixed_b_median_below_a_min": faster}), flush=True)
    if not ok or not faster:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
