"""Several engine calls pending at once behind one delay (tests/stream_order.py): the decode
slots, the upload ring wrapping onto copies that have not run, scratch that regrows under a
pending call, one plan / verifier used from two streams, and a plan destroyed with its work
still queued.  Every call has its own inputs, decoys and output buffers and all are checked, with
no device synchronize before the end.  A call that has to wait on the host for pending device
work (a decode slot, a full ring, a rebind, a destroy) returns when the delay runs out, so the
stream is checked for being pending at the last point before that."""
import numpy as np
import pytest
import torch

import order_cases as C
import rs2_oracle as O
from stream_order import Input, Output, Sandwich, run_checked

pytestmark = pytest.mark.gpu

AXES = ["primary", "secondary"]
RUNS = 5   # objects made ahead: the warm-up pass and up to four delayed runs


def _dev():
    return torch.device("cuda", 0)


def _inp(real, d1, d2, name, stream=None):
    return Input(real, d1, d2, _dev(), stream=stream, name=name)


def _out(ref, name, stream=None):
    ref = np.ascontiguousarray(ref).reshape(-1).view(np.uint8)
    return Output(ref.size, ref, _dev(), stream=stream, name=name)


def _go(label, S, inputs, outputs, call, check=None, join=()):
    rec = run_checked(Sandwich(S, inputs, outputs, _dev(), join=join), call, label, check)
    assert rec["pending"]
    return rec


def _need(n, axis):
    kp, ks = O.source_symbols_for_n_shards(n)
    return kp if axis == "primary" else ks


# ---- decode slots -------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_streams", [False, True])
@pytest.mark.parametrize("axis", AXES)
def test_five_decodes_on_two_slots(gpu, axis, two_streams):
    """Five decodes of one plan, five subsets, five outputs: the plan has two decode slots, so
    the third call waits on the host for the first (pending is taken after the second).  With
    two_streams, calls 1 and 3 go to a second stream that is not delayed."""
    n, length, s = C.DEPTH_DECODE
    S, S2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    plan = gpu.DevicePlan(n, length)
    assert plan.info.symbol_size == s
    need = _need(n, axis)
    calls = []
    for c in range(5):
        st = S2 if two_streams and c % 2 else None
        e = [C.encoded(n, length, 40 + 3 * c + j) for j in range(3)]   # its own blob and decoys
        slv = _inp(e[0][axis], e[1][axis], e[2][axis], f"slivers {c}", st)
        calls.append((slv, _out(e[0]["blob"], f"blob {c}", st), C.subset(n, need, 10 + c),
                      st or S))
    L = C.encoded(n, length, 40)[axis].shape[1]

    def call(sw):
        for c, (slv, out, sel, st) in enumerate(calls):
            plan.decode_async(axis, sel, slv.ptr, [i * L for i in sel], out.ptr, st.cuda_stream)
            if c == 1:
                sw.mark()

    _go(f"5 decodes {axis} two_streams={two_streams}", S, [c[0] for c in calls],
        [c[1] for c in calls], call)


# ---- the upload ring wraps onto pending copies --------------------------------------------------------
def test_upload_ring_wraps_while_pending(gpu):
    """More than 64 ring uploads queued behind the delay: a wrapped slot's previous copy has not
    run, so the host waits in the slot's completion word (rs2_upload_stats slot 2) -- not in a
    device synchronize -- and every call's table still reaches its own kernels."""
    from walrus_amd.encoding import SliverVerifier, device_memory_stats, upload_stats
    n, s = C.VERIFIER_SHAPES[0]
    axis, count = "primary", 3
    S = torch.cuda.Stream(_dev())
    v = SliverVerifier(n, s, axis)
    path_len = len(O.merkle_proof([b"x"] * n, 0))

    def one(c):
        refs = [C.slivers(n, s, axis, count, 100 + 3 * c + j) for j in range(3)]
        targets = [(c + 3 * i) % n for i in range(count)]
        slv = _inp(refs[0]["data"], refs[1]["data"], refs[2]["data"], f"slivers {c}")
        sym = _out(np.stack([refs[0]["expanded"][i, t] for i, t in enumerate(targets)]),
                   f"symbols {c}")
        prf = _out(C.proofs(refs[0], targets), f"proofs {c}")
        assert prf.ref.numel() == count * path_len * 32
        return slv, sym, prf, targets

    def issue(case):
        slv, sym, prf, targets = case
        v.recovery_symbols_async(count, slv.ptr, targets, sym.ptr, prf.ptr, 0, S.cuda_stream)

    # uploads of one call, on an idle stream
    probe = one(0)
    up0 = upload_stats()["uploads"]
    with torch.cuda.stream(S):
        issue(probe)
    S.synchronize()
    per_call = upload_stats()["uploads"] - up0
    assert per_call >= 1, "recovery_symbols_async no longer uploads through the ring"
    n_calls = 64 // per_call + 2
    free_calls = 64 // per_call        # these cannot wait: 64 slots, all idle at the start
    print("stream-order:", {"label": "ring", "uploads_per_call": per_call, "calls": n_calls})
    cases = [one(c) for c in range(n_calls)]
    seen = []

    def call(sw):
        up, syncs = upload_stats(), device_memory_stats()["syncs"]
        for c, case in enumerate(cases):
            issue(case)
            if c == free_calls - 1:
                sw.mark()
        up1 = upload_stats()
        return (up1["uploads"] - up["uploads"], up1["waits"] - up["waits"],
                device_memory_stats()["syncs"] - syncs)

    def check(res):
        seen.append(res)
        assert res[0] > 64 and res[2] == 0, res

    _go(f"ring wrap: {n_calls} recovery_symbols calls", S, [c[0] for c in cases],
        [o for c in cases for o in c[1:3]], call, check=check)
    assert seen[-1][1] >= 1, f"the ring wrapped onto pending copies without a wait: {seen}"


# ---- scratch that regrows while its last user is pending ----------------------------------------------
@pytest.mark.parametrize("axis", AXES)
def test_verifier_scratch_regrows_while_pending(gpu, axis):
    """roots_async of 2 slivers, then of 40, on a fresh verifier: the second call regrows the
    leaf and repair scratch that the first, still pending, is about to use."""
    from walrus_amd.encoding import SliverVerifier
    n, s = C.VERIFIER_SHAPES[1]
    S = torch.cuda.Stream(_dev())
    fresh = [SliverVerifier(n, s, axis) for _ in range(RUNS)]
    used = []
    parts = []
    for c, count in enumerate((2, 40)):
        refs = [C.slivers(n, s, axis, count, 10 * c + j) for j in range(3)]
        parts.append((count, _inp(refs[0]["data"], refs[1]["data"], refs[2]["data"],
                                  f"slivers x{count}"), _out(refs[0]["roots"], f"roots x{count}")))

    def call(sw):
        v = fresh.pop()
        used.append(v)
        for count, slv, roots in parts:
            v.roots_async(count, slv.ptr, roots.ptr, S.cuda_stream)

    _go(f"scratch regrowth {axis}", S, [p[1] for p in parts], [p[2] for p in parts], call)


# ---- a fresh plan's first call: its tables are bound behind the pending work ---------------------------
@pytest.mark.parametrize("entry", ["encode", "metadata", "split", "decode"])
def test_first_call_of_a_fresh_plan_while_pending(gpu, entry):
    """Every run takes a plan that has not been used: the job tables are planned, uploaded and
    bound by this very call, on a stream that is pending (the one-call sandwiches bind theirs in
    the warm-up pass, on an idle stream)."""
    n, length, s = C.ENCODE_SHAPES[1]
    S, P = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    plans = [gpu.DevicePlan(n, length) for _ in range(RUNS)]
    used = []
    e = C.encoded(n, length, 60)
    if entry == "decode":
        src = _inp(e["primary"], C.encoded(n, length, 61)["primary"],
                   C.encoded(n, length, 62)["primary"], "slivers")
        outs = [_out(e["blob"], "blob")]
        sel = C.subset(n, _need(n, "primary"), 21)
        L = e["primary"].shape[1]
    else:
        src = _inp(e["blob"], C.decoy_blob(n, length, 61), C.decoy_blob(n, length, 62), "blob")
        keys = ("hashes", "blob_id") if entry == "metadata" else \
            ("primary", "secondary", "hashes", "blob_id")
        outs = [_out(e[k], k) for k in keys]
        if entry == "split":
            outs[0].snap_stream = P

    def call(sw):
        plan = plans.pop()
        used.append(plan)
        h = S.cuda_stream
        if entry == "decode":
            plan.decode_async("primary", sel, src.ptr, [i * L for i in sel], outs[0].ptr, h)
        elif entry == "metadata":
            plan.compute_metadata_async(src.ptr, outs[0].ptr, outs[1].ptr, h)
        elif entry == "split":
            plan.encode_split_async(src.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                    h, P.cuda_stream)
        else:
            plan.encode_async(src.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, h)

    _go(f"fresh plan: {entry}", S, [src], outs, call, join=[P] if entry == "split" else ())


# ---- one object, two streams --------------------------------------------------------------------------
def test_one_plan_two_streams(gpu):
    """Blob A encoded on the delayed stream, blob B with the same plan into other buffers on an
    idle second stream: the second encode is ordered behind the first (the plan's enc_done)."""
    n, length, s = C.ENCODE_SHAPES[1]
    S, S2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    plan = gpu.DevicePlan(n, length)
    parts = []
    for c, st in enumerate((None, S2)):
        e = C.encoded(n, length, 70 + 3 * c)
        blob = _inp(e["blob"], C.decoy_blob(n, length, 71 + 3 * c),
                    C.decoy_blob(n, length, 72 + 3 * c), f"blob {c}", st)
        outs = [_out(e[k], f"{k} {c}", st) for k in ("primary", "secondary", "hashes", "blob_id")]
        parts.append((blob, outs, st or S))

    def call(sw):
        for c, (blob, o, st) in enumerate(parts):
            plan.encode_async(blob.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, st.cuda_stream)
            sw.mark()      # the second call re-binds the plan: it may wait for the first

    _go("one plan, two streams", S, [p[0] for p in parts], [o for p in parts for o in p[1]], call)


@pytest.mark.parametrize("axis", AXES)
def test_one_verifier_two_streams(gpu, axis):
    """The same for a verifier's scratch (its done event)."""
    from walrus_amd.encoding import SliverVerifier
    n, s = C.VERIFIER_SHAPES[1]
    S, S2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    v = SliverVerifier(n, s, axis)
    parts = []
    for c, st in enumerate((None, S2)):
        refs = [C.slivers(n, s, axis, 3, 80 + 3 * c + j) for j in range(3)]
        parts.append((_inp(refs[0]["data"], refs[1]["data"], refs[2]["data"], f"slivers {c}", st),
                      _out(refs[0]["roots"], f"roots {c}", st), st or S))

    def call(sw):
        for slv, roots, st in parts:
            v.roots_async(3, slv.ptr, roots.ptr, st.cuda_stream)
            sw.mark()

    _go(f"one verifier, two streams {axis}", S, [p[0] for p in parts], [p[1] for p in parts], call)


# ---- a plan destroyed with its work still queued ------------------------------------------------------
def test_plan_destroyed_while_pending(gpu):
    """An encode and a decode of its primary slivers queued on the delayed stream, the plan
    dropped, and at once a plan of another shape created and run on another stream, where it
    takes the arena ranges the first one gave back.  Both plans' results must be right."""
    n, length, s = C.ENCODE_SHAPES[1]
    n2, length2 = 100, 200_000
    S, S2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    plans = [gpu.DevicePlan(n, length) for _ in range(RUNS)]
    e, e2 = C.encoded(n, length, 90), C.encoded(n2, length2, 93)
    blob = _inp(e["blob"], C.decoy_blob(n, length, 91), C.decoy_blob(n, length, 92), "blob 1")
    o = [_out(e[k], f"{k} 1") for k in ("primary", "secondary", "hashes", "blob_id")]
    back = _out(e["blob"], "decoded blob 1")
    blob2 = _inp(e2["blob"], C.decoy_blob(n2, length2, 94), C.decoy_blob(n2, length2, 95),
                 "blob 2", S2)
    o2 = [_out(e2[k], f"{k} 2", S2) for k in ("primary", "secondary", "hashes", "blob_id")]
    sel = C.subset(n, _need(n, "primary"), 9)
    L = e["primary"].shape[1]

    def call(sw):
        plan = plans.pop()
        plan.encode_async(blob.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, S.cuda_stream)
        plan.decode_async("primary", sel, o[0].ptr, [i * L for i in sel], back.ptr, S.cuda_stream)
        sw.mark()
        del plan                       # rs2_plan_destroy: waits for the plan's work
        plan2 = gpu.DevicePlan(n2, length2)
        plan2.encode_async(blob2.ptr, o2[0].ptr, o2[1].ptr, o2[2].ptr, o2[3].ptr,
                           S2.cuda_stream)
        return plan2

    _go("plan destroyed while pending", S, [blob, blob2], o + [back] + o2, call)
