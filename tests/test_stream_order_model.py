"""The stream-ordering harness's bookkeeping on CPU tensors in program order (its delay is a no-op
there), and the shape facts the GPU ordering tests rely on (tests/order_cases.py), from rs2_oracle
and the C restatement."""
import numpy as np
import torch

import order_cases as C
import rs2_oracle as O
from stream_order import (SENTINEL_A, SENTINEL_B, Delay, Input, Output, Sandwich, run_checked)

CPU = torch.device("cpu")


def _case(size=96):
    """out = in + 1 (mod 256) on one input and one output."""
    rng = np.random.default_rng(size)
    real, d1, d2 = (rng.integers(0, 256, size, dtype=np.uint8) for _ in range(3))
    inp = Input(real, d1, d2, CPU)
    out = Output(size, real + np.uint8(1), CPU)
    return Sandwich(None, [inp], [out], CPU), inp, out


def _kinds(found):
    return sorted({k for k, _ in found})


def test_correct_call_passes():
    sw, inp, out = _case()
    rec = run_checked(sw, lambda sw: out.buf.copy_(inp.buf + 1), "model")
    assert rec["pending"] and rec["ops"] == 0
    assert torch.equal(out.buf, torch.full_like(out.buf, SENTINEL_B))


def test_delay_is_a_no_op_on_cpu():
    d = Delay(CPU)
    gate = d.enqueue(None, 1.0)
    assert gate.ops == 0 and gate.pending()


def test_read_at_call_time_is_flagged():
    """A callee that computes from what the buffer held when the host issued the call (decoy 1:
    the real bytes are still queued behind the delay) -- here modelled by reading the decoy."""
    sw, inp, out = _case()
    sw.run(lambda sw: out.buf.copy_(inp.decoy + 1), 0.0)
    assert _kinds(sw.findings()) == ["snapshot"]


def test_no_write_is_flagged():
    sw, inp, out = _case()
    sw.run(lambda sw: None, 0.0)
    found = sw.findings()
    assert _kinds(found) == ["snapshot"] and "hold sentinel A" in found[0][1]
    assert bool((out.snap == SENTINEL_A).all())


def test_late_write_is_flagged():
    """The write lands after step 7: sentinel B is gone, and the snapshot never saw the result."""
    sw, inp, out = _case()
    sw.run(lambda sw: None, 0.0)
    out.buf.copy_(inp.real + 1)
    assert _kinds(sw.findings()) == ["late-output", "snapshot"]
    # a correct write followed by a second, late one: only the late check fires
    sw, inp, out = _case()
    sw.run(lambda sw: out.buf.copy_(inp.buf + 1), 0.0)
    out.buf[5] = 0
    assert _kinds(sw.findings()) == ["late-output"]


def test_late_input_write_is_flagged():
    sw, inp, out = _case()
    sw.run(lambda sw: out.buf.copy_(inp.buf + 1), 0.0)
    inp.buf[0] ^= 1
    assert _kinds(sw.findings()) == ["late-input"]


def test_select_and_unwritten_regions():
    """An output compared on an index set; bytes the callee is to leave alone inside it are
    sentinel A in the reference."""
    size = 64
    real = np.arange(size, dtype=np.uint8)
    inp = Input(real, real[::-1].copy(), (real + 7).astype(np.uint8), CPU)
    sel = np.arange(0, 48)
    ref = np.concatenate([real[:32], np.full(16, SENTINEL_A, dtype=np.uint8)])
    out = Output(size, ref, CPU, select=sel)
    sw = Sandwich(None, [inp], [out], CPU)
    sw.run(lambda sw: out.buf[:32].copy_(inp.buf[:32]), 0.0)
    assert sw.findings() == []
    sw.run(lambda sw: out.buf[:40].copy_(inp.buf[:40]), 0.0)
    assert _kinds(sw.findings()) == ["snapshot"]


def test_never_pending_fails():
    sw, inp, out = _case()

    def call(sw):
        sw.marked = False       # what a GPU run records when the delay had already run out
        out.buf.copy_(inp.buf + 1)

    try:
        run_checked(sw, call, "model")
    except AssertionError as e:
        assert "never pending" in str(e)
    else:
        raise AssertionError("an unpending run passed")


# ---- shape facts ----------------------------------------------------------------------------
def test_symbol_sizes_as_claimed():
    for n, length, s in C.ENCODE_SHAPES + C.SPLIT_SHAPES + C.DECODE_SHAPES + [C.DEPTH_DECODE]:
        assert C.symbol_size(n, length) == s, (n, length)
        assert C.c_params(n, length)[2] == s
    for n, s, lens in C.BATCH_SHAPES:
        assert len(set(lens)) == 4 and all(C.symbol_size(n, ln) == s for ln in lens)
    n, s, lens = C.DECODE_BATCH
    assert len(set(lens)) == 5 and all(C.symbol_size(n, ln) == s for ln in lens)
    n, length, s = C.ENCODE_SHAPES[0]
    kp, ks = O.source_symbols_for_n_shards(n)
    assert length % 2 == 1 and length < kp * ks * s and length // (ks * s) < kp   # tail rows
    assert C.ENCODE_SHAPES[1][2] > 126 and C.VERIFIER_SHAPES[1][1] > 126          # LDS-window leaves


def test_big_message_shapes():
    kp, ks = O.source_symbols_for_n_shards(100)
    assert (kp, ks) == (34, 67)
    full, part = C.ENCODE_SHAPES[2], C.ENCODE_SHAPES[3]
    assert (full[1], part[1]) == (67_109_880, 67_109_875)
    for n, length, s in (full, part):
        assert s == 29_460 and C.symbol_size(n, length) == s
        assert kp * ks * s == 67_109_880 >= C.BIG_MESSAGE
    # one symbol size less is below the bound: these are the smallest messages of that graph
    assert kp * ks * (29_460 - 2) < C.BIG_MESSAGE
    row = ks * 29_460
    assert full[1] // row == kp                       # every row whole
    assert part[1] // row == 33 < kp                  # a partial last row


def test_c_restatement_equals_oracle_at_n10():
    n, length, s = C.ENCODE_SHAPES[0]
    e = C.encoded(n, length)
    ref = O.encode_with_metadata(e["blob"].tobytes(), n)
    assert (e["kp"], e["ks"], e["s"]) == (ref.params.n_primary, ref.params.n_secondary, s)
    assert np.array_equal(e["primary"], ref.primary)
    assert np.array_equal(e["secondary"], ref.secondary)
    assert e["hashes"].tobytes() == b"".join(p + q for p, q in ref.pair_hashes)
    assert e["blob_id"].tobytes() == ref.blob_id
    # a batch blob and a decoy alike
    for ln in C.BATCH_SHAPES[0][2]:
        e = C.encoded(n, ln, seed=3)
        ref = O.encode_with_metadata(e["blob"].tobytes(), n)
        assert np.array_equal(e["primary"], ref.primary) and e["blob_id"].tobytes() == ref.blob_id


def test_sliver_references_are_consistent():
    n, s = C.VERIFIER_SHAPES[0]
    for axis in ("primary", "secondary"):
        r = C.slivers(n, s, axis, 3)
        k = C.k_of(n, axis)
        assert r["data"].shape == (3, k, s) and r["expanded"].shape == (3, n, s)
        assert np.array_equal(r["expanded"][:, :k], r["data"])
        t = [0, n - 1, n // 2]
        p = C.proofs(r, t)
        path_len = p.size // (3 * 32)
        for i in range(3):
            path = [p[(i * path_len + l) * 32:(i * path_len + l + 1) * 32].tobytes()
                    for l in range(path_len)]
            assert O.merkle_proof_root(path, r["expanded"][i, t[i]].tobytes(), t[i]) == \
                r["roots"][i].tobytes()
        assert not np.array_equal(r["data"], C.slivers(n, s, axis, 3, seed=1)["data"])
    sel = C.subset(100, 34, 5)
    assert len(set(sel)) == 34 and 0 not in sel and max(sel) < 100
