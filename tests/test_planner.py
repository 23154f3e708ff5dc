"""CPU check of the codec job planner (walrus_amd/csrc/rs2_planner.*): tests/capi/planner_check
is built from the planner sources alone with the host compiler (no device runtime, not the
library), plans encodes and decodes for a fixed list of shard counts and erasure patterns,
asserts the properties every correct plan has, and prints one line of scalars and a digest per
plan.  The lines must equal tests/golden/planner_digests.txt.

A change that alters the planner's output on purpose regenerates the golden file
(``tests/capi/build/planner_check > tests/golden/planner_digests.txt``) and shows the diff."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CAPI = ROOT / "tests" / "capi"
GOLDEN = ROOT / "tests" / "golden" / "planner_digests.txt"


def test_planner_output_matches_golden():
    subprocess.run(["make", "-C", str(CAPI), "build/planner_check"], check=True,
                   capture_output=True)
    run = subprocess.run([str(CAPI / "build" / "planner_check")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr  # non-zero: a property of the plans was breached
    got = run.stdout.splitlines()
    want = GOLDEN.read_text().splitlines()
    assert len(want) > 600
    differ = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not differ, differ[:5]
    assert len(got) == len(want)
