"""CPU check of the mixed sliver recovery planner (walrus_amd/csrc/rs2_planner.h:
cut_range_chunks, plan_recover_mixed).  tests/capi/planner_ranges_check.cpp is compiled here with
the host compiler from the planner sources alone (no device runtime, not the library, not the
Makefile), once plainly and once under the host sanitizers, and both programs are run stand-alone.

The program asserts: real windows -- every symbol size of the GPU tests on both axes at n = 10,
13, 100 and 1000, planned as the engine plans them -- cut into at most two block-size classes, one
launch each, nothing demoted, with one tile per job up to 256-byte symbols and two at 258; tile
prefix arrays exact for pairs_span on both sides of a tile edge and for several lines per job; the
table-budget cut and the 2^31 - 1 cut on synthetic job sizes (a job above the budget alone in its
chunk, a job above the grid demoted); every per-sliver refusal in the stated order, with and
without status_out; the whole-call refusals; and the window rule: a budget of one sliver, of two,
the 257th group and the 342nd sliver.  This file adds what must hold per line."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_ranges_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
REAL = re.compile(r"real n=(\d+) slivers=(\d+) batched=(\d+) classes=(\d+) launches=(\d+)$")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_ranges")
    plain, san = out / "planner_ranges_check", out / "planner_ranges_check_san"
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
    return plain, san


def _run(prog):
    run = subprocess.run([str(prog)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]  # non-zero: a property was breached
    return run.stdout.splitlines()


def test_cut_validation_and_windows(programs):
    lines = _run(programs[0])
    for fixed in ("refusals ok", "windows ok", "budget chunks=6", "grid chunks=3 demoted=1",
                  "edges classes=2 tiles=205"):
        assert fixed in lines
    real = {}
    for ln in lines:
        m = REAL.match(ln)
        if m:
            n, slivers, batched, classes, launches = (int(x) for x in m.groups())
            assert 1 <= classes <= 2 and launches == classes, ln
            assert 0 < batched <= slivers, ln
            real.setdefault(n, []).append((slivers, batched, classes))
    assert sorted(real) == [10, 13, 100, 1000]
    # n = 13: the two axes differ in block size, so a window has two classes; the others one
    assert real[13][0][2] == 2 and all(c == 1 for n in (10, 100, 1000) for _, _, c in real[n])
    # every burst pattern of these geometries is batched except where it erases nothing
    assert all(b == s for n in (10, 100, 1000) for s, b, _ in real[n])
    assert (440, 440, 1) in real[100]


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
