"""CPU check of the mixed blob encode planner (walrus_amd/csrc/rs2_planner.h: plan_blob_stages,
plan_blobs_mixed).  tests/capi/planner_blobs_check.cpp is compiled here with the host compiler from
the planner sources alone (no device runtime, not the library, not the Makefile), once plainly and
once under the host sanitizers, and both programs are run stand-alone.

The program asserts, for n in {10, 13, 100, 1000, 4500}, every symbol size of the GPU tests times
their blob lengths, 1 and 5 blobs per (size, length), three caller orders, sliver and metadata-only
calls, and budgets that hold 1, 2 and all blobs of the largest size: the windows partition the blobs
in order and are exactly those of the window rule restated (none could have taken the next blob),
the eligible slots come first and keep the caller's order, each stage's tile prefix is increasing
and equals ceil(n_lines * pairs_span / 64) per job, every offset of a job is the template's times s
and every store it can make lies inside the blob's documented extents (at n <= 100 the stored and
loaded symbol sets are compared whole), and every refusal returns its code.  This file adds what
must hold per line: the window counts, and that every (n, s >= 4) with n <= 4096 is eligible while
s = 2 and n = 4500 are not."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_blobs_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
CASE = re.compile(r"n=(\d+) sizes=(\d+) per=(\d+) order=(\d) hold=(\d+) meta=(\d) blobs=(\d+) "
                  r"windows=(\d+) eligible=(\d+)$")
CAP = re.compile(r"cap n=(\d+) blobs=(\d+) cap=(\d+) windows=(\d+) eligible=(\d+)$")
ELIGIBLE = re.compile(r"eligible n=(\d+) s=(\d+) in=(\d+)/(\d+)/(\d+) out=(\d+)/(\d+)/(\d+) "
                      r"C=(\d+) mode=(\d)/(\d)/(\d) fused=(\d): (\d)$")
SIZES = [2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258]
SIZES_1000 = [2, 20, 66, 130]
NS = (10, 13, 100, 1000, 4500)


def _kinds(n):
    """(size, length) kinds of a call: four lengths per size, and length 1 at n = 10."""
    return 4 * len(SIZES_1000 if n >= 1000 else SIZES) + (1 if n == 10 else 0)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_blobs")
    plain, san = out / "planner_blobs_check", out / "planner_blobs_check_san"
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


def test_windows_tiles_extents_and_refusals(programs):
    lines = _run(programs[0])
    assert "refusals ok" in lines
    cases, caps, eligible = set(), set(), {}
    for ln in lines:
        if ln == "refusals ok":
            continue
        m = ELIGIBLE.match(ln)
        if m:
            v = [int(x) for x in m.groups()]
            eligible[(v[0], v[1])] = v[2:]
            continue
        m = CAP.match(ln)
        if m:
            n, blobs, cap, windows, el = (int(x) for x in m.groups())
            assert blobs == 5 * _kinds(n), ln
            # every window but the last holds `cap` eligible blobs
            assert windows == max(1, -(-el // cap)), ln
            caps.add(n)
            continue
        m = CASE.match(ln)
        assert m, ln
        n, sizes, per, order, hold, meta, blobs, windows, el = (int(x) for x in m.groups())
        assert blobs == per * _kinds(n), ln
        small = per * (5 if n == 10 else 4)  # the blobs of s = 2
        assert el == (0 if n > 4096 else blobs - small), ln
        if hold == 0:
            assert windows == 1, ln
        else:
            # a budget of `hold` blobs of the largest size: no window holds fewer than that many
            # but the last, and none is empty
            assert -(-blobs // (hold * 64)) <= windows <= -(-blobs // hold), ln
        if hold == 1 and order == 1 and per == 5 and not meta:
            # sorted by size: the five blobs of the largest size and length each close a window
            assert windows >= 5 * 4, ln
        cases.add((n, per, order, hold, meta))
    for n in NS:
        assert n in caps
        for per in (1, 5):
            for order in (0, 1, 2):
                for hold in (1, 2, 0):
                    for meta in (0, 1):
                        assert (n, per, order, hold, meta) in cases
    # eligibility: every (n, s >= 4) of the GPU tests' lists; s = 2 and n = 4500 never
    for n in NS:
        for s in (SIZES_1000 if n >= 1000 else SIZES):
            assert eligible[(n, s)][-1] == (1 if s >= 4 and n <= 4096 else 0), (n, s)
    # the geometries the GPU tests rely on (rs2_device.h CodecMode: 0 rows, 1 cols): the column
    # code is a shared-input block with the copy-out fused, but a mixing code at n = 13, where the
    # staging launch writes the systematic secondary slivers
    for n, C in ((10, 4), (100, 64), (1000, 512)):
        v = eligible[(n, 4 if n < 1000 else 20)]
        assert v[:6] == [1, 2, 1, 2, 1, 2] and v[6] == C and v[7:11] == [1, 0, 1, 1], (n, v)
    v = eligible[(13, 4)]
    assert v[7:11] == [0, 0, 0, 0] and v[1] == 3, v
    assert eligible[(4500, 20)][6] == 512 and eligible[(4500, 20)][10] == 0


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
