"""CPU check of the bulk recovery-symbol planner (walrus_amd/csrc/rs2_planner.h:
plan_symbol_requests, merkle_level_bases).  tests/capi/planner_symbols_check.cpp is compiled here
with the host compiler from the planner sources alone (no device runtime, not the library, not the
Makefile), once plainly and once under the host sanitizers, and both programs are run stand-alone.

The program asserts, for n in {10, 100, 1000, 4500}, both sliver axes, s in {2, 6, 1206}, four
count lists (with empty slivers, one with none but empty ones), both tree modes and budgets that
hold 1, 2 and all slivers: the windows partition slivers and requests in order, every packed table
entry decodes to its (slot, target), the runs of slivers to expand are exactly those the mode asks
for, the level bases equal a restatement of merkle.rs padding for n in {4, 7, 10, 100, 1000, 4097,
65535}, and every refusal the planner can see returns its code (the pointer rules -- NULL verifier
or buffer, misalignment -- need the device entry point: tests/test_gpu_symbols_multi_3_guard.py).
This file adds what must hold per line: the window counts, that a CACHED call with systematic
targets never launches the codec, that one with repair targets expands only slivers that have
targets, and that BUILD expands every sliver exactly when the trees go to the caller."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_symbols_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
CASE = re.compile(r"n=(\d+) axis=(\d) s=(\d+) slivers=(\d+) trees=(\d) nodes=(\d) hold=(\d+) "
                  r"targets=(\w+) requests=(\d+) windows=(\d+) expanded=(\d+) codec=(\d)$")
LEVELS = re.compile(r"levels n=(\d+) path_len=(\d+) n_nodes=(\d+)$")
BUILD, CACHED = 0, 1
# sliver counts of the program's four lists -> (slivers with targets, requests)
LISTS = {5: (4, 13), 6: (4, 121), 4: (0, 0), 7: (7, 14)}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_symbols")
    plain, san = out / "planner_symbols_check", out / "planner_symbols_check_san"
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


def test_windows_table_levels_and_refusals(programs):
    lines = _run(programs[0])
    assert "refusals ok" in lines
    levels = {}
    seen = set()
    for ln in lines:
        m = LEVELS.match(ln)
        if m:
            levels[int(m.group(1))] = (int(m.group(2)), int(m.group(3)))
            continue
        if ln == "refusals ok":
            continue
        m = CASE.match(ln)
        assert m, ln
        n, axis, s, slivers, trees, nodes, hold = (int(m.group(k)) for k in range(1, 8))
        kind = m.group(8)
        requests, windows, expanded, codec = (int(m.group(k)) for k in range(9, 13))
        seen.add((n, axis, s, slivers, trees, nodes, hold, kind))
        with_targets, want_requests = LISTS[slivers]
        assert requests == want_requests, ln
        assert windows == (-(-slivers // hold) if hold else 1), ln
        if trees == BUILD:
            assert expanded == (slivers if nodes else with_targets), ln
        elif kind == "systematic":
            assert expanded == 0 and codec == 0, ln
        elif kind == "repair":
            assert expanded == with_targets, ln
        else:  # mixed: a sliver with two or more targets asks for symbol k
            assert expanded <= with_targets, ln
        assert codec == (expanded > 0), ln
    # merkle.rs path_length and n_nodes, by hand for the small trees
    assert levels[4] == (2, 7) and levels[7] == (3, 15) and levels[10] == (4, 23)
    assert levels[65535][0] == 16 and set(levels) == {4, 7, 10, 100, 1000, 4097, 65535}
    for n in (10, 100, 1000, 4500):
        for axis in (0, 1):
            for s in (2, 6, 1206):
                for slivers in LISTS:
                    for trees, nodes in ((BUILD, 0), (BUILD, 1), (CACHED, 1)):
                        for hold in (1, 2, 0):
                            for kind in ("mixed", "systematic", "repair"):
                                assert (n, axis, s, slivers, trees, nodes, hold, kind) in seen


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
