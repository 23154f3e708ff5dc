"""CPU check of the decode-batch planner functions (walrus_amd/csrc/rs2_planner.h:
batch_eligible, pack_batch_job).  tests/capi/planner_batch_check.cpp is compiled here with the
host compiler from the planner sources alone (no device runtime, not the library, not the
Makefile), once plainly and once under the host sanitizers, and both programs are run stand-alone.

The program asserts, for n in {10, 13, 100, 1000, 3100, 4500} on both axes, block limits 512 and
256 (and 128 at n = 1000), seeded random K-subsets plus all-repair, all-systematic and
one-erasure patterns, that batch_eligible equals the rule (a decode with at most 8 blocks each
way, s >= 4, nothing to copy or a covered fused copy-out), that every field of the packed job
equals the planned job's below n_in / n_out, and that each re-strided mixing table equals its
source.  This file adds what must hold per case: never at n = 4500 or n = 1000 / limit 128 for
random subsets, never with 2-byte symbols, never when nothing is erased, always otherwise."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_batch_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
LINE = re.compile(r"n=(\d+) axis=(\d) bm=(\d+) s=(\d+) pat=(\w+) seed=(\d+) n_in=(\d+) n_out=(\d+) "
                  r"originals=(\d+) fused=(\d) eligible=(\d)$")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_batch")
    plain, san = out / "planner_batch_check", out / "planner_batch_check_san"
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


def test_batch_rule_and_packed_jobs(programs):
    lines = _run(programs[0])
    seen = set()
    for ln in lines:
        m = LINE.match(ln)
        assert m, ln
        n, axis, bm, s = (int(m.group(k)) for k in range(1, 5))
        pat, n_in, n_out, eligible = m.group(5), int(m.group(7)), int(m.group(8)), int(m.group(11))
        seen.add((n, axis, bm, pat))
        if s < 4 or pat == "all_systematic":
            assert not eligible, ln
        elif pat == "random" and (n == 4500 or (n == 1000 and bm == 128)):
            assert not eligible and max(n_in, n_out) > 8, ln
        elif pat in ("random", "all_repair") and ((n <= 3100 and bm == 512) or
                                                   (n <= 1000 and bm == 256)):
            assert eligible and n_in <= 8 and n_out <= 5, ln
    for n in (10, 13, 100, 1000, 3100, 4500):
        for axis in (0, 1):
            for bm in (512, 256) + ((128,) if n == 1000 else ()):
                for pat in ("random", "all_repair", "all_systematic", "one_erasure"):
                    assert (n, axis, bm, pat) in seen


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
