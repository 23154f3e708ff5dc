"""CPU check of the mixed recovery-symbol planner (walrus_amd/csrc/rs2_planner.h:
plan_symbols_mixed).  tests/capi/planner_symbols_mixed_check.cpp is compiled here with the host
compiler from the planner sources alone (no device runtime, not the library, not the Makefile),
once plainly and once under the host sanitizers, and both programs are run stand-alone.

The program asserts, for n in {10, 13, 100, 1000, 4500}, eleven slivers alternating between the
axes over one symbol size and over five (2, 4, 6, 18, 258), three count lists (one of them all
zero), both tree modes and budgets that hold one sliver, two and all of them: the windows partition
slivers and requests in the caller's order by the restated rule; every accepted sliver has one
slot, the expanded ones first and grouped, the others in the caller's order; every table entry
decodes to its (slot, target) and a refused sliver's entries are the skip mark; the per-slot first
requests are right; the expanded set is exactly what BUILD (with and without trees for the caller)
and CACHED ask for; the groups' tile prefix arrays are consistent; 600 groups are cut at the 257th;
the per-sliver refusals come in the stated order, with and without status_out; the whole-call
refusals, the 65535-sliver cap and the 2^31-1 request cap (on synthetic counts, before any target
is read).  This file adds what must hold per line."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_symbols_mixed_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
CASE = re.compile(r"n=(\d+) slivers=(\d+) sizes=(\d+) trees=(\d) nodes=(\d) hold=(\d+) "
                  r"targets=(\w+) requests=(\d+) windows=(\d+) expanded=(\d+)$")
BUILD, CACHED = 0, 1
# requests of eleven slivers cycling through the program's three count lists -> slivers with targets
LISTS = {29: 9, 0: 0, 22: 11}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_symbols_mixed")
    plain, san = out / "planner_symbols_mixed_check", out / "planner_symbols_mixed_check_san"
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


def test_windows_slots_table_and_refusals(programs):
    lines = _run(programs[0])
    assert "refusals ok" in lines and "group cap windows=3" in lines
    seen = set()
    for ln in lines:
        m = CASE.match(ln)
        if not m:
            assert ln in ("refusals ok", "group cap windows=3"), ln
            continue
        n, slivers, sizes, trees, nodes, hold = (int(m.group(k)) for k in range(1, 7))
        kind = m.group(7)
        requests, windows, expanded = (int(m.group(k)) for k in range(8, 11))
        seen.add((n, sizes, requests, trees, nodes, hold, kind))
        with_targets = LISTS[requests]
        if hold == 0:
            assert windows == 1, ln
        elif sizes == 1:
            assert windows == -(-slivers // hold), ln
        else:  # smaller sizes pack tighter than the largest, never looser
            assert 1 <= windows <= -(-slivers // hold), ln
        if trees == BUILD:
            assert expanded == (slivers if nodes else with_targets), ln
        elif kind == "systematic":
            assert expanded == 0, ln
        elif kind == "repair":
            assert expanded == with_targets, ln
        else:  # mixed: a sliver with two or more targets asks for symbol K
            assert expanded <= with_targets, ln
    for n in (10, 13, 100, 1000, 4500):
        for sizes in (1, 5):
            for requests in LISTS:
                for trees, nodes in ((BUILD, 0), (BUILD, 1), (CACHED, 1)):
                    for hold in (1, 2, 0):
                        for kind in ("mixed", "systematic", "repair"):
                            assert (n, sizes, requests, trees, nodes, hold, kind) in seen


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
