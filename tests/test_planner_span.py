"""The planner's span rule on the CPU, for exactly the calls the far-stride GPU tests make.

finish_plan and sliver_pairs_span (walrus_amd/csrc/rs2_planner.cpp) give a codec job an even
pairs_span while its largest line stride is below T = (2^31 - 65536) / 64 = 33,553,408 bytes and a
multiple of 64 from T on; the kernels' 32-bit per-lane offsets rely on it.  tests/capi/
planner_span_check.cpp is compiled here with the host compiler from rs2_planner.cpp alone (no
device runtime, not the library, not the Makefile), once plainly and once under the host
sanitizers, and both programs are run stand-alone on the call descriptions of tests/
test_gpu_far_1_codec1d.py (every code, size and stride case) and the (axis, size) groups of tests/
test_gpu_far_2_slivers.py.  This file restates the rule, asserts every printed pairs_span against
it, and asserts that each case list holds both kinds of span and that the sliver sizes sit one
step either side of the switch -- so the GPU files cannot drift off the branch they claim to run."""
import re
import subprocess
from pathlib import Path

import pytest

import test_gpu_far_1_codec1d as F1
import test_gpu_far_2_slivers as F2

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_span_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
T = (2 ** 31 - 65536) // 64
LINE = re.compile(r"(\d+) (?:copy|span=(\d+) pairs=(\d+) max_ls=(\d+))$")


def span_rule(n_pairs, max_ls):
    """The rule restated: even below T, a multiple of 64 from T on."""
    return (n_pairs + 63) // 64 * 64 if max_ls >= T else (n_pairs + 1) // 2 * 2


def codec_calls():
    out = []
    for k, n, _, _ in F1.PAIRS:
        for s in F1.SIZES:
            for group in F1.GROUPS:
                out += F1.encode_calls(k, n, s, group) + F1.decode_calls(k, n, s, group)
    for s in F1.SIZES:
        out += F1.symbol_stride_calls(s)
    return out


def sliver_groups():
    return [(a, s) for a in F2.AXES for s in F2.LARGE[a] + F2.SMALL]


def describe(c):
    k, r = c["k"], c["n"] - c["k"]
    if c["op"] == "enc":
        return f"enc {k} {r} {c['s']} {c['src_ss']} {c['src_ls']} {c['dst_ss']} {c['dst_ls']}"
    pairs = " ".join(f"{q} {o}" for q, o in zip(c["idx"], c["sym_off"]))
    return (f"dec {k} {r} {c['s']} {c['src_ls']} {c['out_ss']} {c['out_ls']} {c['limit']} "
            f"{len(c['idx'])} {pairs}")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_span")
    plain, san = out / "planner_span_check", out / "planner_span_check_san"
    builds = [
        subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wall", "-o", str(plain), *SRC, "-lpthread"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
        subprocess.Popen(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-o", str(san), *SRC, "-lpthread"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
    ]
    for b in builds:
        log, _ = b.communicate()
        assert b.returncode == 0, log
    cases = out / "cases.txt"
    lines = [describe(c) for c in codec_calls()]
    lines += [f"grp {F2.N} {F2.AXES.index(a)} {s}" for a, s in sliver_groups()]
    cases.write_text("\n".join(lines) + "\n")
    return plain, san, cases


def _run(prog, cases):
    run = subprocess.run([str(prog), str(cases)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    return run.stdout.splitlines()


def test_every_call_gets_the_span_the_rule_says(programs):
    plain, _, cases = programs
    calls, groups = codec_calls(), sliver_groups()
    lines = _run(plain, cases)
    assert len(lines) == len(calls) + len(groups)
    kinds = {}
    for at, (ln, c) in enumerate(zip(lines, calls + groups), 1):
        m = LINE.match(ln)
        assert m and int(m.group(1)) == at, ln
        if at > len(calls):      # a sliver group: the job's line stride is max(K, n - K) * s
            axis, s = c
            k = F2.k_of(axis)
            max_ls, where = max(k, F2.N - k) * s, ("slivers", axis)
        else:
            s, where = c["s"], (c["op"], c["tag"].split(" ")[0])
            max_ls = max(c["src_ls"], c["dst_ls"] if c["op"] == "enc" else c["out_ls"])
            used = [q for q in dict.fromkeys(c.get("idx", [c["k"]])) if q < c["n"]][:c["k"]]
            if all(q < c["k"] for q in used):
                assert ln == f"{at} copy", (ln, c["tag"])   # every source present: no codec job
                continue
        span, pairs, got_ls = (int(x) for x in m.groups()[1:])
        assert pairs == (s + 3) // 4 and got_ls == max_ls, (ln, c)
        assert span == span_rule(pairs, max_ls), (ln, c)
        assert span >= pairs and span % 2 == 0
        kinds.setdefault(where, set()).add("64" if max_ls >= T else "even")
    # the line-stride groups sit where they claim, encode and decode alike
    for op in ("enc", "dec"):
        assert kinds[(op, "Tm2")] == {"even"}
        assert kinds[(op, "T")] == {"64"}          # one far side makes the job's span
        assert kinds[(op, "2p31")] == {"64"}
    assert kinds[("slivers", "primary")] == kinds[("slivers", "secondary")] == {"even", "64"}
    # a far symbol stride leaves the line stride, and so the span, small
    assert all(kinds[(op, t)] == {"even"} for op, t in
               (("enc", "src_sym_stride"), ("enc", "repair_sym_stride"), ("dec", "sym_off"),
                ("dec", "out_sym_stride")))


def test_far_side_alone_decides(programs):
    """Per call of the T and 2^31 groups: 64-multiple span exactly when a far side is in it."""
    for k, n, _, _ in F1.PAIRS:
        for s in F1.SIZES:
            for group in ("T", "2p31"):
                for c in F1.encode_calls(k, n, s, group) + F1.decode_calls(k, n, s, group):
                    ls = max(c["src_ls"], c.get("dst_ls", 0), c.get("out_ls", 0))
                    assert ls >= T and span_rule((s + 3) // 4, ls) % 64 == 0
            for c in F1.encode_calls(k, n, s, "Tm2") + F1.decode_calls(k, n, s, "Tm2"):
                ls = max(c["src_ls"], c.get("dst_ls", 0), c.get("out_ls", 0))
                assert ls == T - 2 and span_rule((s + 3) // 4, ls) == (s + 3) // 4 + (s + 3) // 4 % 2
    # at s = 2 under the even span a 64-pair tile takes 32 lines: 34 lines make it span 0 .. 31
    assert span_rule(1, T - 2) == 2 and 64 // span_rule(1, T - 2) == 32 < 34


def test_sliver_sizes_sit_one_step_either_side_of_the_switch():
    for axis in F2.AXES:
        k = F2.k_of(axis)
        far = max(k, F2.N - k)
        below, above, top = F2.LARGE[axis]
        assert far * below < T <= far * (below + 2) and above == below + 2
        assert span_rule((below + 3) // 4, far * below) == (below + 3) // 4 + (below + 3) // 4 % 2
        assert span_rule((above + 3) // 4, far * above) % 64 == 0
        assert span_rule((top + 3) // 4, far * top) == 16384
        for s in F2.SMALL:
            assert far * s < T
    # the production figures of the header: 667 * 50,304 < T <= 667 * 50,306
    assert 667 * 50304 < T <= 667 * 50306 and 666 * 50380 < T <= 666 * 50382


def test_same_under_host_sanitizers(programs):
    plain, san, cases = programs
    assert _run(san, cases) == _run(plain, cases)
