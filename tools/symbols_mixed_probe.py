#!/usr/bin/env python3
"""Mixed recovery symbols against the per-size loop (the measurement behind DESIGN.md §21).

At n = 1000, `--slivers` (128) seeded random source slivers with `--targets` (10) seeded targets
each, half of them systematic.  Every argument is marshalled and every verifier created before the
clock starts; each repetition is timed from the first call to the stream's completion (wall clock,
synchronised at both ends), the two paths alternating, one warm-up of each, `--reps` repetitions,
every one checked byte-equal (symbols, proofs, and with BUILD the trees) to the other path's:
 (A) mixed: 64 distinct even symbol sizes spread over 4 .. 300, two slivers each, the sizes
     alternating between the two axes
     (a) the loop a caller writes without the mixed call: one
         rs2_verifier_recovery_symbols_multi_device_async per (axis, size) on the same stream
     (b) one rs2_sliver_checker_recovery_symbols_device_async call (also: the time until it returns)
 (B) uniform: every sliver primary at s = 1206
     (a) one rs2_verifier_recovery_symbols_multi_device_async call   (b) one mixed call
Both with RS2_TREES_BUILD into d_nodes and with RS2_TREES_CACHED from it.  (a) is the reference of
each case.  Exits non-zero when a result is wrong, or when (A b) does not beat (A a) by more than
the wider of the two min-max spreads in either mode; (B) has no pass mark, its ratio says which
call a uniform batch should use.  Prints one JSON line (and writes it to --out).
usage: python3 tools/symbols_mixed_probe.py [--slivers 128] [--targets 10] [--reps 9] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from walrus_amd import _lib
    from walrus_amd.encoding import SliverChecker, SliverVerifier, _stream, symbols_mixed_stats
    n, M, T = 1000, args.slivers, args.targets
    f = (n - 1) // 3
    K = {"primary": n - f, "secondary": n - 2 * f}
    AX = {"primary": 0, "secondary": 1}
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stp = _stream(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(42)
    checker = SliverChecker(n)
    L, nn = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.rs2_merkle_tree_shape(n, ctypes.byref(L), ctypes.byref(nn)) == 0
    L, nn = L.value, nn.value
    u8, u16, u32, u64 = ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64
    BUILD, CACHED = _lib.RS2_TREES_BUILD, _lib.RS2_TREES_CACHED

    def setup(slivers):
        """slivers: [(axis, s)], sorted by group so that a group's slivers, symbols, proofs and
        trees are neighbours and path (a) can hand a group to its verifier in one call."""
        slivers = sorted(slivers, key=lambda x: (x[1], AX[x[0]]))
        m = len(slivers)
        in_off, out_off, targets, ia, oa = [], [], [], 0, 0
        for axis, s in slivers:
            k = K[axis]
            ts = [int(t) for t in rng.integers(0, k, T // 2)] + \
                 [int(t) for t in rng.integers(k, n, T - T // 2)]
            targets.append([ts[i] for i in rng.permutation(T)])
            in_off.append(ia)
            out_off.append(oa)
            ia += k * s
            oa += T * s
        d_in = torch.from_numpy(rng.integers(0, 256, ia, dtype=np.uint8)).to(dev)
        groups = []                       # (verifier, first sliver, count)
        for i, (axis, s) in enumerate(slivers):
            if groups and slivers[groups[-1][1]] == (axis, s):
                groups[-1][2] += 1
            else:
                groups.append([SliverVerifier(n, s, axis), i, 1])
        flat = [t for ts in targets for t in ts]
        a = {"m": m, "groups": groups, "d_in": d_in,
             "ax": (u8 * m)(*[AX[x[0]] for x in slivers]), "sz": (u16 * m)(*[x[1] for x in slivers]),
             "io": (u64 * m)(*in_off), "oo": (u64 * m)(*out_off), "in_off": in_off,
             "out_off": out_off, "cnt": (u32 * m)(*([T] * m)), "tg": (u16 * len(flat))(*flat),
             "sym_b": oa}
        # per group: its own count and target arrays (marshalled before the clock starts)
        a["garr"] = [((u32 * c)(*([T] * c)), (u16 * (c * T))(*flat[i0 * T:(i0 + c) * T]))
                     for _, i0, c in groups]
        return a

    def outputs(a):
        return (torch.zeros(a["sym_b"], dtype=torch.uint8, device=dev),
                torch.zeros(a["m"] * T * L * 32, dtype=torch.uint8, device=dev),
                torch.zeros(a["m"] * nn * 32, dtype=torch.uint8, device=dev))

    def loop(a, trees, out):
        sym, prf, nodes = out
        for (v, i0, c), (cnt, tg) in zip(a["groups"], a["garr"]):
            rc = lib.rs2_verifier_recovery_symbols_multi_device_async(
                v.handle, c, a["d_in"].data_ptr() + a["in_off"][i0], cnt, tg, trees,
                nodes.data_ptr() + i0 * nn * 32, sym.data_ptr() + a["out_off"][i0],
                prf.data_ptr() + i0 * T * L * 32, stp)
            assert rc == 0, _lib.last_error()
        return None

    def mixed(a, trees, out):
        sym, prf, nodes = out
        rc = lib.rs2_sliver_checker_recovery_symbols_device_async(
            checker.handle, a["m"], ctypes.cast(a["ax"], ctypes.c_void_p), a["sz"],
            a["d_in"].data_ptr(), a["io"], a["cnt"], a["tg"], trees, nodes.data_ptr(),
            sym.data_ptr(), a["oo"], prf.data_ptr(), None, stp)
        assert rc == 0, _lib.last_error()
        return time.perf_counter()

    def timed(fn, a, trees, out):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = fn(a, trees, out)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, ((ret - t0) * 1e3 if ret else None)

    def summary(xs):
        xs = sorted(xs)
        return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4),
                "max_ms": round(xs[-1], 4)}

    def case(slivers):
        a = setup(slivers)
        out_a, out_b = outputs(a), outputs(a)
        res = {"groups": len(a["groups"])}
        ok = True
        for trees, name in ((BUILD, "build"), (CACHED, "cached")):
            ta, tb, ret = [], [], []
            for rep in range(args.reps + 1):      # repetition 0 is the warm-up of each path
                if trees == BUILD:
                    for o in out_a + out_b:
                        o.zero_()
                else:
                    for o in out_a[:2] + out_b[:2]:
                        o.zero_()
                before = symbols_mixed_stats()
                x, _ = timed(loop, a, trees, out_a)
                y, r = timed(mixed, a, trees, out_b)
                after = symbols_mixed_stats()
                same = all(torch.equal(p, q) for p, q in zip(out_a, out_b))
                nonzero = bool(out_a[0].any()) and bool(out_a[1].any()) and bool(out_a[2].any())
                if not (same and nonzero):
                    ok = False
                if rep:
                    ta.append(x), tb.append(y), ret.append(r)
            res[name] = {"loop": summary(ta), "mixed": summary(tb),
                         "mixed_returns_ms": round(sorted(ret)[len(ret) // 2], 4),
                         "ratio": round(summary(ta)["median_ms"] / summary(tb)["median_ms"], 3),
                         "counters": {k: after[k] - before[k] for k in after}}
        return res, ok

    sizes = [4 + 2 * int(round(i * (300 - 4) / 2 / 63)) for i in range(64)]
    assert len(set(sizes)) == 64 and sizes[0] == 4 and sizes[-1] == 300
    per = max(M // 64, 1)
    mixed_list = [(("primary", "secondary")[i % 2], s) for i, s in enumerate(sizes)] * per
    res_a, ok_a = case(mixed_list[:M])
    res_b, ok_b = case([("primary", 1206)] * M)
    passed = ok_a and ok_b
    for name in ("build", "cached"):
        lo, mx = res_a[name]["loop"], res_a[name]["mixed"]
        spread = max(lo["max_ms"] - lo["min_ms"], mx["max_ms"] - mx["min_ms"])
        res_a[name]["margin_ms"] = round(lo["median_ms"] - mx["median_ms"], 4)
        res_a[name]["spread_ms"] = round(spread, 4)
        passed = passed and lo["median_ms"] - mx["median_ms"] > spread
    line = json.dumps({"n_shards": n, "slivers": M, "targets": T, "reps": args.reps,
                       "bytes_equal": ok_a and ok_b, "A_mixed_64_sizes": res_a,
                       "B_uniform_s1206": res_b, "pass": passed})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if passed else 1


if __name__ == "__main__":
    sys.exit(main())
