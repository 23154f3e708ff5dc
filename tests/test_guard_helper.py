"""tests/guarded.py on CPU tensors: a stray write into either guard or into a stride gap is
reported (with its offset relative to the payload), and a clean buffer passes -- so the
containment tests built on it can fail."""
import numpy as np
import pytest
import torch

from guarded import DELTAS, GUARD, Guarded, pattern, strided_extents, strided_mask


def test_layout_and_pattern():
    for delta in DELTAS:
        g = Guarded(100, delta, "cpu", fill=7)
        assert g.buf.numel() == 4096 + delta + 100 + 4096 and g.buf.dtype == torch.uint8
        assert g.ptr == g.buf.data_ptr() + 4096 + delta == g.payload.data_ptr()
        assert g.ptr % 16 == delta and g.payload.numel() == 100
        i = np.arange(g.buf.numel())
        assert np.array_equal(g.buf.numpy(), ((i * 131 + 7) & 0xFF).astype(np.uint8))
    assert not torch.equal(pattern(64, 1), pattern(64, 2))
    assert Guarded(0, 2).payload.numel() == 0


def test_clean_run_passes():
    g = Guarded(64, 6, "cpu", fill=3)
    g.assert_guards_intact()
    g.payload.fill_(0xEE)              # the whole payload is writable without extents
    g.assert_guards_intact()
    g.set(np.arange(10, dtype=np.uint8), offset=54)
    assert g.numpy()[54:].tolist() == list(range(10))
    g.assert_guards_intact()


@pytest.mark.parametrize("delta", [0, 2, 14])
def test_stray_write_in_a_guard_is_reported(delta):
    g = Guarded(64, delta, "cpu", fill=5)
    g.buf[g.start - 1] ^= 0x01          # the last front-guard byte
    with pytest.raises(AssertionError, match=r"payload offset -1 \(front guard"):
        g.assert_guards_intact(what="out")
    g = Guarded(64, delta, "cpu", fill=5)
    g.buf[g.start + 64] ^= 0x80         # the first back-guard byte
    with pytest.raises(AssertionError, match=r"payload offset 64 \(back guard"):
        g.assert_guards_intact()
    g = Guarded(64, delta, "cpu", fill=5)
    g.buf[0] ^= 0xFF                    # the far ends of both guards
    g.buf[-1] ^= 0xFF
    assert g.changed() == [-GUARD - delta, 64 + GUARD - 1]


def test_stray_write_in_a_stride_gap_is_reported():
    # 3 lines of 4 symbols of 6 bytes, symbol stride 8, line stride 40 (gaps of 2 and of 8)
    ext = strided_extents(3, 40, 4, 8, 6)
    size = 2 * 40 + 3 * 8 + 6
    assert ext[:2] == [(0, 6), (8, 6)] and ext[-1] == (size - 6, 6) and len(ext) == 12
    mask = strided_mask(size, 3, 40, 4, 8, 6)
    for extents in (ext, mask):
        g = Guarded(size, 4, "cpu", fill=9)
        for off, ln in ext:
            g.payload[off:off + ln] = 0xAB
        g.assert_guards_intact(extents)
        g.payload[6] ^= 0x10            # first byte of the gap after symbol 0
        with pytest.raises(AssertionError, match=r"payload offset 6 \(gap"):
            g.assert_guards_intact(extents)
        g.assert_guards_intact()        # ... which the whole-payload check cannot see
    g = Guarded(size, 4, "cpu", fill=9)
    g.payload[32 + 5] ^= 0x10           # the gap between two lines
    assert g.changed(mask) == [37]


def test_limit_cuts_the_writable_extents():
    ext = strided_extents(2, 20, 2, 8, 6, limit=25)
    assert ext == [(0, 6), (8, 6), (20, 5)]
    mask = strided_mask(34, 2, 20, 2, 8, 6, limit=25)
    assert np.flatnonzero(mask).tolist() == list(range(6)) + list(range(8, 14)) + list(range(20, 25))
    g = Guarded(34, 0, "cpu", fill=1)
    g.payload[25] ^= 1                  # the first byte at the limit, inside a symbol
    with pytest.raises(AssertionError, match="payload offset 25"):
        g.assert_guards_intact(mask)
    assert strided_extents(1, 0, 2, 6, 6, limit=0) == []
    with pytest.raises(AssertionError):
        Guarded(10, 0).changed([(8, 4)])   # an extent past the payload is a test bug
