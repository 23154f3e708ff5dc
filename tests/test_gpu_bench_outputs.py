"""bench.py's plain run and --dump-outputs (GPU): one small run of the real command.  The line
holds the metric with the timed steps as asked and no side leg; the dumped arrays are float32 and
are the step's outputs: the decoded blob is the seeded input, and slivers, hashes and BlobId
equal the host API's encode of that blob."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BLOB_LEN, STEPS = 10, 1 << 19, 3  # every dumped array is below bench.DUMP_SAMPLE: kept whole
LEGS = ("cpu_baseline", "host_io", "host_abi", "c1_c2_split", "c3_small_blobs", "c4_partitioned",
        "quilt", "node_side")


def test_plain_run_line_and_dump(gpu, tmp_path):
    import torch
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", str(STEPS), "--warmup", "1", "--n-shards", str(N),
                          "--blob-mib", str(BLOB_LEN / (1 << 20)), "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u16"
    assert d["ms_per_step"] > 0
    # value = blob bytes per second of the timed steps, in GiB/s (both are rounded in the line)
    gibs = BLOB_LEN / (1 << 30) / (d["ms_per_step"] / 1e3)
    assert d["value"] == pytest.approx(gibs, rel=1e-2, abs=2e-3)
    assert all(d[k] is None for k in LEGS) and d["decode_roundtrip_ok"] is None
    assert d["stages_ms_solo"] is None and "solo" not in (d["roofline"] or {})

    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["blob_id", "decoded_blob", "primary_slivers", "secondary_slivers",
                           "sliver_pair_hashes"]
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)  # bench.py's blob on rank 0
    blob = torch.randint(0, 256, (BLOB_LEN,), dtype=torch.uint8, device=dev, generator=g)
    blob = blob.cpu().numpy()
    assert np.array_equal(got["decoded_blob"], blob.astype(np.float32))
    pairs, meta = gpu.ReedSolomonEncodingConfig(N).encode_with_metadata(blob.tobytes())

    def f32(b):
        return np.frombuffer(b, dtype=np.uint8).astype(np.float32)
    assert np.array_equal(got["blob_id"], f32(bytes(meta.blob_id)))
    assert np.array_equal(got["sliver_pair_hashes"], f32(meta.metadata.hashes_bytes()))
    assert np.array_equal(got["primary_slivers"],
                          f32(b"".join(p.primary.symbols.data for p in pairs)))
    # the device buffer holds the secondary slivers by sliver index; pair i carries n - 1 - i
    assert np.array_equal(got["secondary_slivers"],
                          f32(b"".join(p.secondary.symbols.data for p in reversed(pairs))))
