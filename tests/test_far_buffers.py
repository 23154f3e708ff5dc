"""tests/far_buffers.py on CPU tensors, checked the way test_guard_helper.py checks Guarded: a
stray byte planted in a window, in a gap between symbols and past out_limit is each reported with
its offset, a clean buffer passes, and a whole buffer also sees what a sparse one cannot -- so the
far-stride tests built on it can fail."""
import numpy as np
import pytest
import torch

from far_buffers import CHUNK, GUARD, FarBuffer, Grid, line_runs, merge_windows
from guarded import pattern

LS = 40000      # line stride: the lines' windows (run + 2 * 4 KiB) do not meet


def _buf(whole, delta=6, lines=3, fill=9):
    # per line 4 symbols of 6 bytes, symbol stride 8 (gaps of 2)
    grid = Grid(lines, LS, 4, 8, 6)
    assert grid.size == (lines - 1) * LS + 3 * 8 + 6
    return FarBuffer(grid.size, line_runs(lines, LS, 30), delta, "cpu", fill, whole=whole), grid


def test_windows_merge_and_clip():
    assert merge_windows([(100, 10)], 0, 1000, pad=20) == [(80, 130)]
    assert merge_windows([(100, 10), (10, 5)], 0, 1000, pad=20) == [(0, 35), (80, 130)]
    assert merge_windows([(100, 10), (140, 10)], 0, 1000, pad=20) == [(80, 170)]     # touch
    assert merge_windows([(100, 10), (120, 10)], 0, 125, pad=20) == [(80, 125)]      # overlap, clip
    assert merge_windows([(0, 0), (50, 0)], -8, 58, pad=4) == [(-4, 4), (46, 54)]


@pytest.mark.parametrize("delta", [0, 6, 14])
def test_layout_and_pattern(delta):
    b, grid = _buf(False, delta)
    assert b.buf.numel() == GUARD + delta + grid.size + GUARD
    assert b.ptr == b.payload.data_ptr() and b.ptr % 16 == delta and b.payload.numel() == grid.size
    # windows: front guard + line 0, line 1, line 2 + back guard; the pattern is Guarded's
    assert b.windows == [(-GUARD - delta, 30 + GUARD), (LS - GUARD, LS + 30 + GUARD),
                         (2 * LS - GUARD, grid.size + GUARD)]
    want = pattern(b.total, 9)
    for lo, hi in b.windows:
        assert torch.equal(b.buf[lo + b.start:hi + b.start], want[lo + b.start:hi + b.start])
    w, _ = _buf(True, delta)
    assert torch.equal(w.buf, want)
    assert w.whole and not b.whole and FarBuffer(10, [(0, 10)]).whole   # the size rule: small = whole


@pytest.mark.parametrize("whole", [False, True])
def test_clean_run_passes(whole):
    b, grid = _buf(whole)
    b.assert_intact()
    b.assert_intact(grid)
    snap = b.snapshot()
    b.view(grid)[:] = 0xAB              # every documented byte written
    b.assert_intact(grid, "out")
    assert b.payload[8:14].tolist() == [0xAB] * 6 and b.payload[LS + 24] == 0xAB
    with pytest.raises(AssertionError, match="written at payload offset 0"):
        b.assert_unchanged(snap)
    assert len(b.changed()) == 3 * 4 * 6     # ... which an input's check (no grid) reports


@pytest.mark.parametrize("whole", [False, True])
def test_stray_bytes_are_reported_with_their_offsets(whole):
    b, grid = _buf(whole)
    b.view(grid)[:] = 0xAB
    b.payload[6] ^= 0x10                 # the gap after symbol 0 of line 0
    with pytest.raises(AssertionError, match=r"payload offset 6 \(gap"):
        b.assert_intact(grid)
    b.payload[LS + 30 + 100] ^= 1        # in line 1's window, past its run
    b.payload[2 * LS - 1] ^= 1           # before line 2
    b.buf[b.start - 1] ^= 1              # the last front-guard byte
    b.buf[0] ^= 0x80                     # the far ends of both guards
    b.buf[-1] ^= 0x80
    assert b.changed(grid) == [-b.start, -1, 6, LS + 130, 2 * LS - 1, grid.size + GUARD - 1]
    g = FarBuffer(grid.size, line_runs(3, LS, 30), 2, "cpu", 5, whole=whole)
    g.buf[g.start + grid.size] ^= 1      # the first back-guard byte
    with pytest.raises(AssertionError, match=rf"payload offset {grid.size} \(back guard"):
        g.assert_intact(grid, "out")
    f = FarBuffer(grid.size, line_runs(3, LS, 30), 2, "cpu", 5, whole=whole)
    f.buf[f.start - 3] ^= 1
    with pytest.raises(AssertionError, match=r"payload offset -3 \(front guard"):
        f.assert_intact(grid, "out")


def test_between_the_windows_only_a_whole_buffer_sees():
    at = LS // 2                         # 4 KiB and more from every run
    sparse, grid = _buf(False)
    sparse.payload[at] = 1               # uninitialised there: no pattern to compare with
    assert sparse.changed(grid) == []
    whole, _ = _buf(True)
    whole.payload[at] ^= 1
    assert whole.changed(grid) == [at]
    with pytest.raises(AssertionError, match=rf"payload offset {at} \(gap.*whole\)"):
        whole.assert_intact(grid)


@pytest.mark.parametrize("whole", [False, True])
def test_limit_cuts_the_writable_extents(whole):
    limit = LS + 8 + 3                   # inside symbol 1 of line 1, at an odd byte
    grid = Grid(3, LS, 4, 8, 6, limit)
    assert np.flatnonzero(grid.mask(LS - 2, LS + 16)).tolist() == [2, 3, 4, 5, 6, 7, 10, 11, 12]
    assert np.flatnonzero(grid.mask(-5, 9)).tolist() == [5, 6, 7, 8, 9, 10, 13]
    assert not grid.mask(2 * LS - 10, 2 * LS + 30).any()
    b = FarBuffer(grid.size, line_runs(3, LS, 30), 4, "cpu", 1, whole=whole)
    v = b.view(grid)
    v[0] = 0xCD
    v[1, 0] = 0xCD
    v[1, 1, :3] = 0xCD
    b.assert_intact(grid)
    b.payload[limit] ^= 1                # the first byte at the limit, inside a symbol
    with pytest.raises(AssertionError, match=rf"payload offset {limit} \(at or past out_limit"):
        b.assert_intact(grid)
    b.payload[2 * LS + 8] ^= 1           # a symbol of the last line, wholly past the limit
    assert b.changed(grid) == [limit, 2 * LS + 8]
    with pytest.raises(AssertionError):
        FarBuffer(10, [(8, 4)])          # a run past the payload is a test bug
    with pytest.raises(AssertionError):
        Grid(2, 4, 2, 4, 6)              # overlapping symbols too


def test_chunked_over_more_than_one_chunk():
    """A window and a gap longer than one 16 MiB step: the pattern continues across the steps
    and a byte in each step is found."""
    size = 2 * CHUNK + 12345
    for whole, runs in ((False, [(0, size)]), (True, [(0, 16), (size - 16, 16)])):
        b = FarBuffer(size, runs, 10, "cpu", 77, whole=whole)
        assert torch.equal(b.buf[CHUNK - 5:CHUNK + 300], pattern(CHUNK + 300, 77)[CHUNK - 5:])
        assert b.changed() == []
        b.payload[5] ^= 1
        b.payload[CHUNK + 1] ^= 1
        b.payload[size - 20] ^= 1
        assert b.changed() == [5, CHUNK + 1, size - 20]
