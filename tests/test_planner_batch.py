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
random subsets, never with 2-byte symbols, never when nothing is erased, always otherwise.

Given a file of explicit patterns the program runs those through the same checks instead.  The
last test feeds it every family pattern of the geometries of the batched GPU tests
(tests/erasure_patterns.py BATCH_GEOMETRIES and BLOB_300) and compares what the planner made of
each with the Python restatement that those tests predict their paths from."""
import hashlib
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = [str(ROOT / "tests" / "capi" / "planner_batch_check.cpp"),
       str(ROOT / "walrus_amd" / "csrc" / "rs2_planner.cpp")]
LINE = re.compile(r"n=(\d+) axis=(\d) bm=(\d+) s=(\d+) pat=(\w+) seed=(\d+) n_in=(\d+) n_out=(\d+) "
                  r"originals=(\d+) fused=(\d) eligible=(\d)$")
FILE_LINE = re.compile(r"line=(\d+) k=(\d+) n=(\d+) bm=(\d+) s=(\d+) n_in=(\d+) n_out=(\d+) "
                       r"originals=(\d+) fused=(\d) eligible=(\d) paired=(\d+)$")
# SHA-256 of the program's output without an argument (338 lines), as it was before the file form
BUILT_IN_OUTPUT = "8c20ccd49768a82583bd74b80be80b8fd76998a24b14d416d54f3631d5fbb9ef"


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


def _run(prog, *args):
    run = subprocess.run([str(prog), *map(str, args)], capture_output=True, text=True)
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


def test_built_in_cases_unchanged(programs):
    run = subprocess.run([str(programs[0])], capture_output=True)
    assert run.returncode == 0 and run.stderr == b"planner_batch_check: 338 cases\n"
    assert hashlib.sha256(run.stdout).hexdigest() == BUILT_IN_OUTPUT


def test_chunk_cut_rule(programs):
    """cut_batch_chunks, the rule that packs a window's eligible jobs into launches, on the
    smallest windows at which it can go wrong (`--chunks`; jobs of 3 logs = 768 table bytes, one of
    7 logs = 1792).  The program checks for each that every eligible job is in exactly one chunk or
    demoted and no other job in either, that a chunk has one geometry and stays within the budget
    unless it is a single job; the expected cuts below are what the loop this rule replaced (in
    decode_batch_items and recover_items) gives: demotion against the chunk's first job, the cut
    before the job that would pass the budget, a demoted job's tables not counted."""
    expected = {
        "empty": ("-", "-"),
        "none_eligible": ("-", "-"),
        "three_fit": ("0,1,2", "-"),
        "three_exact": ("0,1,2", "-"),             # the budget itself is not past the budget
        "two_fit": ("0,1|2", "-"),                 # the cut falls before the job that overflows
        "one_above_budget": ("0", "-"),            # still a chunk of its own
        "above_budget_between": ("0|1|2", "-"),
        "other_c_between": ("0,2", "1"),           # demoted; its neighbours share one chunk
        "other_span_between": ("0,2", "1"),
        "ineligible_first": ("1,3", "2"),          # the first eligible job defines the geometry
        "demoted_does_not_count": ("0,2|3", "1"),
        "geometry_of_each_chunk": ("0,1|2", "3"),  # compared with the open chunk's first job
        "zero_budget": ("0|1", "-"),
    }
    lines = _run(programs[0], "--chunks")
    got = {}
    for ln in lines:
        m = re.fullmatch(r"(\w+) chunks=(\S+) demoted=(\S+)", ln)
        assert m, ln
        got[m.group(1)] = (m.group(2), m.group(3))
    assert got == expected
    assert _run(programs[1], "--chunks") == lines   # the same under the host sanitizers


def test_families_of_the_batch_geometries(programs, tmp_path):
    """Every family pattern of every BATCH_GEOMETRIES entry (s = 6) through the program's file
    form, plain and under the host sanitizers: the planner's n_in, n_out and eligibility equal
    decode_layout / batch_path, "the planner paired" equals pair_precondition, and the fused copy
    of the present originals is covered wherever an original is present (so the engine's
    `originals > 0 && !fused` fallback does not occur in the batched GPU tests)."""
    from erasure_patterns import (BATCH_GEOMETRIES, BLOB_300, batch_path, decode_layout, families,
                                  pair_precondition)
    s = 6
    cases = []
    geometries = BATCH_GEOMETRIES + BLOB_300   # (BLOB_300: what the GPU calls run at n = 300)
    for k, n, limit, count, eligible in geometries:
        fams = families(k, n, limit)
        assert len(fams) == count
        cases += [(k, n, limit, name, present) for name, present in fams]
    path = tmp_path / "families.txt"
    path.write_text("".join(f"{k} {n} {limit} {s} {' '.join(map(str, present))}\n"
                            for k, n, limit, _, present in cases))
    lines = _run(programs[0], path)
    assert len(lines) == len(cases) == 776 + 255
    eligible_seen, paired_seen = {}, 0
    for at, (ln, (k, n, limit, name, present)) in enumerate(zip(lines, cases), 1):
        m = FILE_LINE.match(ln)
        assert m, ln
        got = dict(zip(("line", "k", "n", "bm", "s", "n_in", "n_out", "originals", "fused",
                        "eligible", "paired"), map(int, m.groups())))
        what = f"{k}-of-{n} block limit {limit} pattern {name}: {ln}"
        assert (got["line"], got["k"], got["n"], got["bm"], got["s"]) == (at, k, n, limit, s), what
        lay = decode_layout(k, n, limit, present)
        assert (got["n_in"], got["n_out"]) == (len(lay.in_blocks), len(lay.out_blocks)), \
            f"{what}\n{lay}"
        assert got["eligible"] == (batch_path(lay, s) == "batched"), f"{what}\n{lay}"
        assert got["originals"] == k - len(lay.erased), what
        assert got["paired"] == int(pair_precondition(lay)), f"{what}\n{lay}"
        assert got["fused"] == int(got["originals"] > 0), what
        eligible_seen[k, n, limit] = eligible_seen.get((k, n, limit), 0) + got["eligible"]
        paired_seen += got["paired"]
    assert eligible_seen == {(k, n, limit): e for k, n, limit, _, e in geometries}
    assert paired_seen == 180 + 26
    assert _run(programs[1], path) == lines
