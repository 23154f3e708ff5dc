#!/usr/bin/env python3
"""Mixed sliver recovery against the per-size loop (the measurement behind DESIGN.md §20).

At n = 1000, `--slivers` (128) seeded random slivers, each recovered from a fresh random K-subset
of its 1000 recovery symbols handed over in random order.  Every argument is marshalled and every
verifier created before the clock starts; each repetition is timed from the first call to the
stream's completion (wall clock, synchronised at both ends), the two paths alternating, one
warm-up of each, `--reps` repetitions, every one checked for all-MATCH verdicts and exact slivers:
 (A) mixed: 64 distinct even symbol sizes spread over 4 .. 300, two slivers each, the sizes
     alternating between the two axes
     (a) the loop a caller writes without the mixed call: one
         rs2_verifier_recover_slivers_device_async per (axis, size) on the same stream
     (b) one rs2_sliver_checker_recover_device_async call (also: the time until it returns)
 (B) uniform: every sliver primary at s = 1206
     (a) one rs2_verifier_recover_slivers_device_async call   (b) one mixed call
(a) is the reference of each case.  Exits non-zero when a result is wrong, or when (A b) does not
beat (A a) by more than the wider of the two min-max spreads; (B) has no pass mark, its ratio says
which call a uniform batch should use.  Prints one JSON line (and writes it to --out).
usage: python3 tools/recover_mixed_probe.py [--slivers 128] [--reps 7] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverChecker, SliverVerifier, _stream, recover_mixed_stats
    n, M = 1000, args.slivers
    f = (n - 1) // 3
    K = {"primary": n - f, "secondary": n - 2 * f}
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stp = _stream(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(42)
    checker = SliverChecker(n)

    def setup(slivers):
        """slivers: [(axis, s)].  The symbol buffer holds every sliver's K received symbols back
        to back, the slivers of one (axis, size) neighbours in it, so that path (a) can hand a
        group to its verifier in one call; outputs are laid out the same way."""
        order = sorted(range(len(slivers)), key=lambda i: (slivers[i][1], slivers[i][0]))
        m = len(slivers)
        sym_off, out_off, idx, want = [0] * m, [0] * m, [None] * m, [None] * m
        chunks, at = [], 0
        for i in order:
            axis, s = slivers[i]
            k = K[axis]
            data = rng.integers(0, 256, k * s, dtype=np.uint8)
            cw = np.empty(n * s, dtype=np.uint8)
            assert lib.rs2_encode_1d(k, n, s, 1, data.ctypes.data, cw.ctypes.data) == 0
            pick = rng.permutation(n)[:k]
            idx[i] = [int(q) for q in pick]
            chunks.append(cw.reshape(n, s)[pick].reshape(-1))
            want[i] = data
            sym_off[i] = out_off[i] = at
            at += k * s
        d_sym = torch.from_numpy(np.concatenate(chunks)).to(dev)
        d_want = torch.from_numpy(np.concatenate([want[i] for i in order])).to(dev)
        # expected roots: the engine's own roots of the true slivers (checked against the oracle by
        # the test suite), through one mixed verification call
        d_roots = torch.zeros(m * 32, dtype=torch.uint8, device=dev)
        rc = checker.verify_async([a for a, _ in slivers], [s for _, s in slivers],
                                  d_want.data_ptr(), out_off, None, d_roots.data_ptr(), 0,
                                  torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        expected = np.ascontiguousarray(d_roots.cpu().numpy())
        # path (a): one verifier call per (axis, size) run of neighbours
        runs = []
        for i in order:
            if runs and slivers[runs[-1]["first"]] == slivers[i]:
                runs[-1]["members"].append(i)
            else:
                runs.append({"first": i, "members": [i]})
        for r in runs:
            axis, s = slivers[r["first"]]
            mem = r["members"]
            flat = [q for i in mem for q in idx[i]]
            r.update(v=SliverVerifier(n, s, axis), count=len(mem),
                     counts=(ctypes.c_uint32 * len(mem))(*[len(idx[i]) for i in mem]),
                     idx=(ctypes.c_uint16 * len(flat))(*flat), off=sym_off[r["first"]],
                     exp=np.ascontiguousarray(np.concatenate([expected[32 * i:32 * i + 32] for i in mem])),
                     roots=torch.zeros(len(mem) * 32, dtype=torch.uint8, device=dev),
                     verdict=torch.zeros(len(mem), dtype=torch.int32, device=dev))
        flat = [q for i in range(m) for q in idx[i]]
        return {"m": m, "sym": d_sym, "want": d_want, "runs": runs,
                "out": torch.zeros(at, dtype=torch.uint8, device=dev),
                "verdict": torch.zeros(m, dtype=torch.int32, device=dev),
                "axes": (ctypes.c_uint8 * m)(*[0 if a == "primary" else 1 for a, _ in slivers]),
                "sizes": (ctypes.c_uint16 * m)(*[s for _, s in slivers]),
                "counts": (ctypes.c_uint32 * m)(*[len(x) for x in idx]),
                "idx": (ctypes.c_uint16 * len(flat))(*flat),
                "s_off": (ctypes.c_uint64 * m)(*sym_off), "o_off": (ctypes.c_uint64 * m)(*out_off),
                "exp": expected}

    def loop(c):
        base, out = c["sym"].data_ptr(), c["out"].data_ptr()
        for r in c["runs"]:
            rc = lib.rs2_verifier_recover_slivers_device_async(
                r["v"].handle, r["count"], r["counts"], r["idx"], base + r["off"],
                r["exp"].ctypes.data, out + r["off"], r["roots"].data_ptr(), r["verdict"].data_ptr(),
                None, stp)
            if rc:
                return rc
        return 0

    def mixed(c):
        return lib.rs2_sliver_checker_recover_device_async(
            checker.handle, c["m"], c["axes"], c["sizes"], c["counts"], c["idx"],
            c["sym"].data_ptr(), c["s_off"], c["exp"].ctypes.data, c["out"].data_ptr(), c["o_off"],
            None, c["verdict"].data_ptr(), None, stp)

    def timed(c, fn):
        c["out"].zero_()
        c["verdict"].zero_()
        for r in c["runs"]:
            r["verdict"].zero_()
        torch.cuda.synchronize()
        before = recover_mixed_stats()
        t0 = time.perf_counter()
        rc = fn(c)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, _lib.last_error()
        after = recover_mixed_stats()
        verdicts = c["verdict"] if fn is mixed else torch.cat([r["verdict"] for r in c["runs"]])
        ok = bool(torch.equal(c["out"], c["want"])) and bool((verdicts == 1).all())
        return dt, (t1 - t0) * 1e3, ok, {x: after[x] - before[x] for x in after}

    def summary(xs):
        med = sorted(xs)[len(xs) // 2]
        return {"median_ms": round(med, 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
                "spread_ms": round(max(xs) - min(xs), 3)}

    def compare(c):
        ok = timed(c, loop)[2]                              # warm-up of each
        ok = timed(c, mixed)[2] and ok
        res = {"a": [], "b": []}
        host, stats = [], {}
        for _ in range(args.reps):
            dt, _, good, _ = timed(c, loop)
            res["a"].append(dt)
            ok = ok and good
            dt, h, good, stats = timed(c, mixed)
            res["b"].append(dt)
            host.append(h)
            ok = ok and good
        a, b = summary(res["a"]), summary(res["b"])
        return {"a_per_size": a, "b_mixed": b,
                "b_returns_ms_median": round(sorted(host)[len(host) // 2], 3),
                "a_over_b": round(a["median_ms"] / b["median_ms"], 2),
                "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
                "per_size_calls": len(c["runs"]), "stats_per_call": stats, "ok": ok}

    distinct = [4 + 2 * ((i * 148) // 63) for i in range(64)]   # 64 even sizes over 4 .. 300
    assert len(set(distinct)) == 64 and min(distinct) == 4 and max(distinct) == 300
    per = max(1, M // 64)
    case_a = [(("primary", "secondary")[i % 2], s) for i, s in enumerate(distinct)
              for _ in range(per)]
    mix = compare(setup(case_a))
    uni = compare(setup([("primary", 1206)] * M))
    a, b = mix["a_per_size"], mix["b_mixed"]
    margin = max(a["spread_ms"], b["spread_ms"])
    faster = a["median_ms"] - b["median_ms"] > margin
    ok = mix["ok"] and uni["ok"]
    line = json.dumps({"n": n, "slivers": M, "reps": args.reps, "mixed_64_sizes_both_axes": mix,
                       "uniform_primary_s1206": uni, "ok": ok,
                       "mixed_b_beats_a_by_more_than_the_spreads": faster})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not ok or not faster:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
