"""CPU check of the sliver-recovery planner functions (walrus_amd/csrc/rs2_planner.h:
select_recovery_symbols, sliver_recover_spec).  tests/capi/planner_recover_check.cpp is compiled
here with the host compiler from the planner sources alone (no device runtime, not the library,
not the Makefile), once plainly and once under the host sanitizers, and both programs are run
stand-alone.

The program asserts, for n in {10, 13, 100, 1000, 3100, 4500}, both sliver axes (K_s symbols for a
primary sliver, K_p for a secondary one), s in {2, 6, 20, 1206} and the received-symbol lists
named below, that the selection's status and chosen list equal a direct restatement of the rule
and that every field of the DecodeSpec is the one-line decode of the sliver.  This file adds what
must hold per case: the plan is a batch job whenever something is erased, s >= 4 and n <= 3100;
never at s = 2, never when nothing is erased, never for random subsets at n = 4500."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_recover_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
LINE = re.compile(r"n=(\d+) axis=(\d) s=(\d+) pat=(\w+) seed=(\d+) count=(\d+) rc=(-?\d+) "
                  r"originals=(\d+) n_in=(\d+) n_out=(\d+) eligible=(\d)$")
RS2_OK, NOT_ENOUGH_SHARDS, DECODING_UNSUCCESSFUL = 0, -5, -6
PATTERNS = ("random", "all_repair", "all_original", "one_erasure", "noisy", "one_short",
            "duplicate")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = tmp_path_factory.mktemp("planner_recover")
    plain, san = out / "planner_recover_check", out / "planner_recover_check_san"
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


def test_selection_spec_and_batch_rule(programs):
    lines = _run(programs[0])
    seen = set()
    for ln in lines:
        m = LINE.match(ln)
        assert m, ln
        n, axis, s = (int(m.group(k)) for k in range(1, 4))
        pat, rc, originals = m.group(4), int(m.group(7)), int(m.group(8))
        n_in, n_out, eligible = int(m.group(9)), int(m.group(10)), int(m.group(11))
        seen.add((n, axis, s, pat))
        f = (n - 1) // 3
        K = n - f if axis == 0 else n - 2 * f
        if pat == "one_short":
            assert rc == DECODING_UNSUCCESSFUL and not eligible, ln
            continue
        if pat == "duplicate":
            assert rc == NOT_ENOUGH_SHARDS and not eligible, ln
            continue
        assert rc == RS2_OK, ln
        erased = K - originals
        if pat == "all_original":
            assert erased == 0
        else:
            assert erased > 0, ln  # random and noisy lists leave out original 0
        if s == 2 or erased == 0:
            assert not eligible, ln
        elif n <= 3100:
            assert eligible and 1 <= n_in <= 8 and 1 <= n_out <= 8, ln
        elif pat == "random":
            assert not eligible and max(n_in, n_out) > 8, ln
    for n in (10, 13, 100, 1000, 3100, 4500):
        for axis in (0, 1):
            for s in (2, 6, 20, 1206):
                for pat in PATTERNS:
                    assert (n, axis, s, pat) in seen


def test_same_under_host_sanitizers(programs):
    assert _run(programs[1]) == _run(programs[0])
