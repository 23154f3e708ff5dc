"""The corruption model and its case families, on the CPU (tests/corruption.py).

What the GPU verdict tests rely on is proven here without a device: the model passes its own
test body, the body catches the faults it exists for (an engine that always answers with the
honest result, one that answers with the previous call's result, one that looks at byte 0 of a
sliver only), and every geometry has enough cases on both sides of every verdict.
"""
from collections import Counter

import numpy as np
import pytest

import corruption as C
import rs2_oracle as O

SMALL = ["G0_0", "G0_1", "G1", "G2", "G3", "G4"]


def test_geometries():
    """The symbol sizes and the padding facts the table in corruption.py claims."""
    for g in C.GEOMETRIES.values():
        p = O.Rs2Params.for_blob(g.n, g.length)
        assert p.symbol_size == g.symbol_size, g.id
    row = lambda gid: (lambda p: p.n_secondary * p.symbol_size)(
        O.Rs2Params.for_blob(C.GEOMETRIES[gid].n, C.GEOMETRIES[gid].length))
    assert row("G1") == 42 and 150 - 3 * 42 == 24            # symbols 4..6 of row 3 are padding
    assert 2 * 42 < 113 < 3 * 42 and (113 - 84) % 6 == 5     # row 2 ends mid-element, row 3 empty
    assert row("G3") == 594 and (2901 - 4 * 594) % 66 == 63  # last row ends inside a symbol
    assert 33 * row("G4") < 293001 < 34 * row("G4")
    assert 400001 // row("G5") == 299                        # rows 300..333 are empty
    assert C.symbol_offsets(2) == [0, 1]
    assert C.symbol_offsets(6) == [0, 1, 2, 3, 5]
    assert C.symbol_offsets(66) == [0, 1, 31, 32, 63, 64, 65]
    assert C.symbol_offsets(130) == [0, 1, 31, 32, 63, 64, 128, 129]


def test_layouts():
    """Every layout holds in-range, right-sized slivers; the standard one has a duplicate at
    position 2 and a systematic surplus after exactly K distinct used slivers."""
    for gid, g in C.GEOMETRIES.items():
        p = O.Rs2Params.for_blob(g.n, g.length)
        for name, (axis, idx) in C.layouts(gid).items():
            k = p.n_primary if axis == C.PRIMARY else p.n_secondary
            assert all(0 <= i < g.n for i in idx)
            if name in ("pri", "sec"):
                assert idx[2] == idx[0] and idx[-1] == 0 and len(idx) == k + 2
                used = idx[:2] + idx[3:-1]
                assert len(set(used)) == k and idx[0] < k <= used[-1]
                assert any(i >= k for i in used[1:-1]) or k < 4
            elif name.endswith("_sys"):
                assert idx == tuple(range(k)) + (g.n - 1,)
            else:
                erased = [i for i in range(k) if i not in idx]
                assert len(idx) == k and len(erased) == 1 and sum(i >= k for i in idx) == 1


def test_issue_example_g1():
    """Primary decode from slivers {0, 1, 2, 9} at G1, one bit of sliver 9 flipped: in symbols
    4..6 the flip lands in the padding of row 3 and Default and Strict return the honest blob;
    in symbols 1 or 3 it changes row 3 and both reject."""
    sc = C.scenario("G1")
    s = sc.geo.symbol_size
    for sym, accept in ((4, True), (5, True), (6, True), (1, False), (3, False)):
        for off, mask in ((0, 0x01), (s - 1, 0x80)):
            d = bytearray(sc.sliver(C.PRIMARY, 9))
            d[sym * s + off] ^= mask
            slivers = [(i, sc.sliver(C.PRIMARY, i)) for i in (0, 1, 2)] + [(9, bytes(d))]
            for check in ("default", "strict"):
                got = C.model_decode_and_verify(10, 150, C.PRIMARY, slivers, sc.hashes,
                                                sc.blob_id, check)
                assert got == (("ok", sc.blob) if accept else ("rejected",)), (sym, off, check)


@pytest.mark.parametrize("gid", SMALL)
def test_model_passes_the_body(gid):
    """The model, run as the engine (its own decode for every call), passes run_sequence."""
    cases = C.cases(gid)
    if gid == "G4":   # a fresh numpy decode per call at n = 100: every third corruption, 3 checks
        cases = [c for i, c in enumerate(cases) if (i // 3) % 3 == 0]
    counts = C.run_sequence(C.model_call, cases)
    assert counts["ok"] + counts["rejected"] == len(cases)
    assert counts["honest"] >= len(cases) // 4 + 2


def _always_honest(case):
    return ("ok", C.scenario(case.geo, case.scen).blob)


class _Stale:
    """Answers every call with the result of the call before it."""

    def __init__(self, first):
        self.last = first

    def __call__(self, case):
        out, self.last = self.last, C.model_call(case)
        return out


def _byte0_only(case):
    """Sees a flip only where it sits in byte 0 of the sliver."""
    return C.model_call(case if case.pos < 0 or case.byte == 0 else
                        C.Case(case.geo, case.scen, case.layout, case.check,
                               hash_edit=case.hash_edit, id_edit=case.id_edit, dlen=case.dlen))


@pytest.mark.parametrize("gid", ["G1", "G3"])
def test_injected_faults_fail_the_body(gid):
    cases = C.cases(gid)
    sc = C.scenario(gid)
    with pytest.raises(AssertionError):
        C.run_sequence(_always_honest, cases)
    with pytest.raises(AssertionError):
        C.run_sequence(_Stale(("ok", sc.blob)), cases)
    with pytest.raises(AssertionError):
        C.run_sequence(_byte0_only, cases)
    # the stale engine is caught by the honest calls too: per layout, with honest_every = 1
    for _, group in C.groups(cases):
        if any(C.expected(c)[0] == "rejected" for c in group):
            with pytest.raises(AssertionError):
                C.run_sequence(_Stale(("ok", sc.blob)), group, honest_every=1)


def _tally(gid):
    t = {chk: Counter() for chk in C.CHECKS}
    accepted_families = {chk: Counter() for chk in C.CHECKS}
    for c in C.cases(gid):
        v = C.expected(c)[0]
        t[c.check][v] += 1
        if v == "ok":
            accepted_families[c.check][c.family + "/" + c.target.split(" ")[0]] += 1
    return t, accepted_families


@pytest.mark.parametrize("gid", list(C.GEOMETRIES))
def test_share_conditions(gid):
    """From the model alone: Skip accepts everything; for G1..G4 Default and Strict each reject
    at least a quarter of the corrupt cases and accept at least three."""
    t, fam = _tally(gid)
    total = sum(t["skip"].values())
    print(f"{gid}: {total} corrupt cases per check; " + "; ".join(
        f"{chk}: {t[chk]['ok']} accept / {t[chk]['rejected']} reject" for chk in C.CHECKS))
    for chk in ("default", "strict"):
        print(f"  {chk} accepts: {dict(fam[chk])}")
    assert t["skip"]["rejected"] == 0
    if gid in ("G1", "G2", "G3", "G4"):
        for chk in ("default", "strict"):
            assert 4 * t[chk]["rejected"] >= total, (chk, t[chk])
            assert t[chk]["ok"] >= 3, (chk, t[chk])
            # what must be accepted is: padding, surplus and duplicate under both checks
            for f in ("padding/cell", "sliver/surplus", "sliver/duplicate"):
                assert fam[chk][f] >= 1, (chk, f)
        assert fam["default"]["sliver/all"] >= 1             # a verified row is not re-checked
        assert fam["default"]["metadata/hash"] >= 1          # the hashes Default never reads
        assert fam["strict"]["metadata/hash"] >= 1           # Strict reads no hash at all
    if gid != "G0_0":
        # the padding family has both sides: an absorbed flip and its rejected neighbour
        pad = [c for c in C.cases(gid) if c.family == "padding" and c.check != "skip"]
        assert {C.expected(c)[0] for c in pad} == {"ok", "rejected"}


def test_length_cases():
    """A length one short with the same symbol size: Default accepts the shorter blob exactly
    when the lost byte is zero (the padding is zero again) and the row is checked at all;
    Strict always rejects, because the id hashes the length."""
    for gid in ("G1", "G3"):
        for c in C.cases(gid):
            if c.dlen and c.check != "skip":
                want = C.expected(c)
                blob = C.scenario(gid, c.scen).blob
                if c.check == "strict":
                    assert want == ("rejected",)
                elif c.scen == "ztail":
                    assert want == ("ok", blob[:-1])
                else:
                    assert want == ("rejected",), c.describe()


def test_c_model_agrees_with_numpy():
    """The C restatement the model uses from n = 100 gives the numpy model's answers (G3)."""
    cases = C.cases("G3")
    for c in cases[::7]:
        m = C.materialise(c)
        args = (m["n"], m["length"], m["axis"], m["slivers"], m["hashes"], m["blob_id"],
                m["check"])
        assert C.model_decode_and_verify(*args, be=C.backend(0, "c_decode")) == \
            C.model_decode_and_verify(*args, be=C.backend(0, "numpy")), c.describe()


def test_c_sliver_root_agrees_with_numpy():
    """corruption.sliver_root switches to rs2cpu_sliver_root at n = 100: the same roots as the
    numpy oracle there, on both axes, for an honest and a flipped sliver."""
    sc = C.scenario("G4")
    for axis in (C.PRIMARY, C.SECONDARY):
        for byte, mask in C.sliver_positions(sc.params, axis)[::5]:
            d = bytearray(sc.sliver(axis, 41))
            d[byte] ^= mask
            want = O.sliver_merkle_root(np.frombuffer(bytes(d), np.uint8), axis, sc.params)
            assert C.sliver_root(sc.params, axis, bytes(d)) == want
        assert C.sliver_root(sc.params, axis, sc.sliver(axis, 41)) == \
            sc.hashes[sc.pair_of(axis, 41)][axis == C.SECONDARY]
