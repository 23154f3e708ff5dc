"""rs2_blob_encoder_encode_device_async against the oracle: one call over blobs that share only
n_shards -- every symbol size of the list times four lengths (exact, an odd tail, nearly all of the
last symbols padding, an end inside a row and a symbol; at n = 10 also one byte) -- in three caller
orders, with 1 and 5 blobs per kind.  Slivers, pair hashes and ids must equal
oracle.encode_with_metadata; at n = 1000 they are compared with the per-blob device encode, which
the goldens pin.  The sizes cover the codec's 64-byte chunk edges, leaf messages of one, two and
three Blake2b blocks, and s = 6, where several lines share a codec tile.

The same inputs under budgets of one and two blobs must give identical outputs; metadata only must
give the same hashes and ids; the counters must show that no eligible blob took the per-blob path
and that a window costs at most RS2_ENCODE_MIXED_WINDOW_LAUNCHES launches whatever it holds; the
s = 2 blobs and one n = 4500 blob take the per-blob path inside the same call and still match."""
import pytest
import torch

import encode_mixed as M

pytestmark = pytest.mark.gpu

NS = (10, 13, 100, 1000)


@pytest.fixture(scope="module")
def encoders(gpu):
    made = {}

    def get(n):
        if n not in made:
            made[n] = gpu.BlobEncoder(n)
        return made[n]
    yield get
    M.set_budget(0)


def _counts(n, items):
    el = sum(M.eligible(n, M.sym(n, x)) for x, _ in items)
    return el, len(items) - el


@pytest.mark.parametrize("order", M.ORDERS)
@pytest.mark.parametrize("per", [1, 5])
@pytest.mark.parametrize("n", NS)
def test_matches_reference(encoders, n, per, order):
    items = M.case(n, M.sizes_of(n), per, order)
    M.set_budget(0)
    before = M.stats()
    out = M.run(encoders(n), n, items)
    assert out.rc == 0
    windows, grouped, single, sizes, launches = M.moved(before)
    M.check(n, out, f"n={n} per={per} {order}")
    el, rest = _counts(n, items)
    # no eligible blob takes the per-blob path; the s = 2 blobs do
    assert (grouped, single) == (el, rest)
    assert windows >= 1 and launches <= windows * M.LAUNCHES
    assert sizes >= len(M.sizes_of(n)) - 1


@pytest.mark.parametrize("n", NS)
def test_launches_do_not_grow_with_the_blobs(encoders, n):
    """One window, 1 or 5 blobs per kind: the launch counter moves by the same amount.  Sorted by
    size the eligible blobs are neighbours in the caller's arrays, so their hashes and ids are
    written in place (7 launches); interleaved with the s = 2 blobs they go through the window's
    scratch and one more launch moves them, however many they are."""
    M.set_budget(0)
    for order, want in (("sorted", M.LAUNCHES - 1), ("interleaved", None)):
        moves = []
        for per in (1, 5):
            items = M.case(n, M.sizes_of(n), per, order)
            before = M.stats()
            out = M.run(encoders(n), n, items)
            assert out.rc == 0
            windows, _, _, _, launches = M.moved(before)
            assert windows == 1, "the default budget holds the whole call"
            moves.append(launches)
        if want is not None:
            assert moves == [want, want], (order, moves)
        assert all(0 < x <= M.LAUNCHES for x in moves), (order, moves)


@pytest.mark.parametrize("per,order", [(1, "interleaved"), (1, "sorted"), (1, "reverse"),
                                       (5, "interleaved")])
@pytest.mark.parametrize("n", NS)
def test_budgets_give_identical_outputs(encoders, n, per, order):
    items = M.case(n, M.sizes_of(n), per, order)
    smax = M.sizes_of(n)[-1]
    M.set_budget(0)
    base = M.run(encoders(n), n, items)
    M.check(n, base, f"n={n} default budget")
    try:
        for hold in (1, 2):
            M.set_budget(hold * M.scratch(n, smax))
            before = M.stats()
            out = M.run(encoders(n), n, items)
            windows, grouped, single, _, launches = M.moved(before)
            assert out.rc == 0
            # every blob needs at most the largest size's scratch: a window holds `hold` or more
            assert len(items) / (hold * 64) <= windows <= -(-len(items) // hold)
            assert windows > 1
            assert launches <= windows * M.LAUNCHES
            assert (grouped, single) == _counts(n, items)
            for a, b in ((out.primary, base.primary), (out.secondary, base.secondary),
                         (out.hashes, base.hashes), (out.ids, base.ids)):
                assert torch.equal(a, b), f"n={n} hold={hold}: outputs differ from the default budget's"
    finally:
        M.set_budget(0)


@pytest.mark.parametrize("n", NS)
def test_metadata_only(encoders, n):
    items = M.case(n, M.sizes_of(n), 1, "interleaved")
    try:
        for hold in (0, 2):
            M.set_budget(hold * M.scratch(n, M.sizes_of(n)[-1], meta_only=True))
            before = M.stats()
            out = M.run(encoders(n), n, items, meta_only=True)
            assert out.rc == 0
            M.check(n, out, f"n={n} metadata only hold={hold}")
            windows, grouped, single, _, launches = M.moved(before)
            assert (grouped, single) == _counts(n, items)
            assert (windows == 1) == (hold == 0) and launches <= windows * M.LAUNCHES
    finally:
        M.set_budget(0)


def test_wide_code_takes_the_per_blob_path(gpu):
    """n_shards = 4500 (trees wider than a workgroup's): every blob runs through the single-blob
    encode inside the call, and matches it."""
    n = 4500
    kp, ks = M.shape(n)
    items = [(4 * kp * ks - 3, 0), (5, 1)]
    enc = gpu.BlobEncoder(n)
    before = M.stats()
    out = M.run(enc, n, items)
    assert out.rc == 0
    windows, grouped, single, _, launches = M.moved(before)
    assert (grouped, single, launches) == (0, 2, 0)
    M.check(n, out, "n=4500")
