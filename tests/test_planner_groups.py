"""CPU check of the mixed sliver verification planner (walrus_amd/csrc/rs2_planner.h:
plan_sliver_axis, plan_sliver_groups).  tests/capi/planner_groups_check.cpp is compiled here with
the host compiler from the planner sources alone (no device runtime, not the library, not the
Makefile), once plainly and once under the host sanitizers, and both programs are run stand-alone.

The program asserts, for n in {10, 13, 100, 1000, 4500}, every symbol size of the GPU tests on both
axes, 1 and 5 slivers per group, three caller orders and budgets that hold 1, 2 and all slivers of
the largest size: the windows partition the slivers in order and none could have taken the next
sliver, the slot permutation is a bijection onto the accepted slivers and stable inside a group,
groups are maximal per (axis, size) inside a window with the eligible ones first, each axis' tile
prefix is increasing and equals ceil(n_lines * pairs_span / 64) per group, and every refusal
returns its code.  This file adds what must hold per line: the window counts of uniform calls, the
group counts of single-window calls, and that every (n, axis, s >= 4) with n <= 4096 is eligible
while s = 2 and n = 4500 are not."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_groups_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
CASE = re.compile(r"n=(\d+) sizes=(\d+) per=(\d+) order=(\d) hold=(\d+) slivers=(\d+) "
                  r"windows=(\d+) groups=(\d+) eligible=(\d+)$")
UNIFORM = re.compile(r"uniform n=(\d+) s=(\d+) slivers=(\d+) hold=(\d+) windows=(\d+)$")
ELIGIBLE = re.compile(r"eligible n=(\d+) axis=(\d) s=(\d+) in=(\d+) out=(\d+) C=(\d+) mode=(\d): (\d)$")
SIZES = [2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258]
SIZES_1000 = [2, 20, 66, 130, 1206]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_groups")
    plain, san = out / "planner_groups_check", out / "planner_groups_check_san"
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


def test_windows_groups_tiles_and_refusals(programs):
    lines = _run(programs[0])
    assert "refusals ok" in lines
    cases, uniform, eligible = set(), set(), {}
    for ln in lines:
        if ln == "refusals ok":
            continue
        m = UNIFORM.match(ln)
        if m:
            n, s, slivers, hold, windows = (int(x) for x in m.groups())
            assert windows == (-(-slivers // hold) if hold else 1), ln
            uniform.add((n, hold))
            continue
        m = ELIGIBLE.match(ln)
        if m:
            n, axis, s, n_in, n_out, C, mode, el = (int(x) for x in m.groups())
            eligible[(n, axis, s)] = (n_in, n_out, C, mode, el)
            continue
        m = CASE.match(ln)
        assert m, ln
        n, sizes, per, order, hold, slivers, windows, groups, el = (int(x) for x in m.groups())
        assert slivers == 2 * sizes * per, ln
        if hold == 0:  # one window: a group per (axis, size)
            assert windows == 1 and groups == 2 * sizes, ln
            want = 0 if n > 4096 else 2 * (sizes - 1)  # all but s = 2
            assert el == want, ln
        else:
            # the largest size alone fills a 1-sliver budget; smaller ones may share a window
            assert -(-slivers // (hold * 16)) <= windows <= slivers, ln
            assert groups >= 2 * sizes, ln
        if hold == 1 and order == 1 and per == 1:
            assert windows >= 2, ln
        cases.add((n, per, order, hold))
    for n in (10, 13, 100, 1000, 4500):
        for hold in (1, 2, 0):
            assert (n, hold) in uniform
            for per in (1, 5):
                for order in (0, 1, 2):
                    assert (n, per, order, hold) in cases
    # eligibility: every (n, axis, s >= 4) of the GPU tests' lists; s = 2 and n = 4500 never
    for n in (10, 13, 100, 1000):
        for axis in (0, 1):
            for s in (SIZES_1000 if n == 1000 else SIZES):
                n_in, n_out, C, mode, el = eligible[(n, axis, s)]
                assert el == (s >= 4), (n, axis, s)
                assert 1 <= n_in <= 3 and 1 <= n_out <= 3, (n, axis, n_in, n_out)
    assert all(v[4] == 0 for (n, _, _), v in eligible.items() if n == 4500)
    # the geometries the GPU tests rely on (rs2_device.h CodecMode: 0 rows, 1 cols)
    assert eligible[(10, 0, 4)][:4] == (2, 1, 4, 0)      # primary, high rate: 2 in, 1 out
    assert eligible[(10, 1, 4)][:4] == (1, 2, 4, 1)      # secondary: shared input
    assert eligible[(13, 0, 4)][3] == 0 and eligible[(13, 1, 4)][3] == 0  # both high rate
    assert max(eligible[(13, a, 4)][0] for a in (0, 1)) == 3
    assert eligible[(100, 0, 4)][2] == 64
    assert eligible[(1000, 0, 20)][:4] == (2, 1, 512, 0)
    assert eligible[(1000, 1, 20)][:4] == (1, 2, 512, 1)


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
