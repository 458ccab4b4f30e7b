"""The upload plan of a GPU decoder's batch (Staging::plan_uploads, through
hjd_debug_upload_plan): which bytes move host -> device, in how many copies and
in what order, from frames given as numbers -- no GPU, nothing staged.

The expectations are worked out by hand from the rules (DESIGN.md s10.1 "One
call, one descriptor"): a header copy; one copy per run of consecutive
host-destuffed frames, from the first's data_off to the last's data_end()
(= data_off + data_bits / 8 + the 64-byte pad, over all its scans); one copy per
raw scan in the staging; caller-pinned raw scans last, a run placed at its
distance in the caller's memory as one span; a latency decoder's batch that is
host-destuffed throughout as two pull segments of 16-byte words instead.
"""
import ctypes

import numpy as np
import pytest

HOST, CALLER, STAGED = 0, 1, 2                       # destuff modes
HDR, DATA, RAW_STAGED, RAW_CALLER = 0, 1, 2, 3       # row kinds
BASE, USED = 1 << 16, 4096                           # where the data area starts; the header's bytes
SRC = 0x7F0000100000                                 # an address in the caller's memory (only compared)


@pytest.fixture(scope="module")
def lib():
    from ocljpegdecoder_amd import _lib
    return _lib.load()


def frame(mode, data_off, data_bits, raw_len, raw_off=0, raw_src=0, more=(0, -1)):
    return [mode, data_off, data_bits, raw_len, raw_off, raw_src, *more]


def plan(lib, frames, latency=False, prepulled=0):
    """(rows, pull segments, pulled, moved, host_bytes); every result passes the cover check."""
    i64p = ctypes.POINTER(ctypes.c_int64)
    f = np.array(frames, np.int64)
    rows, segs, totals = np.zeros((len(frames) + 1, 6), np.int64), np.zeros((4, 2), np.int64), np.zeros(2, np.int64)
    nrows, nsegs, pull = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.hjd_debug_upload_plan(f.ctypes.data_as(i64p), len(frames), BASE, USED, int(latency), prepulled,
                                   rows.ctypes.data_as(i64p), len(rows), ctypes.byref(nrows),
                                   segs.ctypes.data_as(i64p), ctypes.byref(nsegs), ctypes.byref(pull),
                                   totals.ctypes.data_as(i64p))
    assert rc == 0
    rows = [tuple(int(v) for v in r) for r in rows[:nrows.value]]
    segs = [tuple(int(v) for v in s) for s in segs[:nsegs.value]]
    _cover(frames, rows, segs, bool(pull.value), prepulled)
    return rows, segs, bool(pull.value), int(totals[0]), int(totals[1])


def _cover(frames, rows, segs, pull, prepulled):
    """Destinations pairwise disjoint within the blob and within the raw area;
    every frame in exactly one row's [first, last) -- or, pulled, its scans
    inside the data segment, which then stands for all the frames."""
    for area in ((HDR, DATA), (RAW_STAGED, RAW_CALLER)):
        spans = sorted((r[1], r[1] + r[3]) for r in rows if r[0] in area)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    if pull:
        assert rows == [] and len(segs) == 2
        (h0, hn), (d0, dn) = segs
        assert (h0 + hn) * 16 <= d0 * 16
        assert d0 * 16 <= BASE + frames[0][1] + prepulled
        for f in frames:
            assert f[0] == HOST and BASE + f[1] + f[2] // 8 + 64 <= (d0 + dn) * 16
        return
    assert segs == []
    for i in range(len(frames)):
        assert sum(r[4] <= i < r[5] for r in rows) == 1, (i, rows)


def test_one_host_frame(lib):
    rows, segs, pull, moved, host = plan(lib, [frame(HOST, 128, 8000, 1010)])
    end = 128 + 1000 + 64
    assert not pull
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE + 128, BASE + 128, end - 128, 0, 1)]
    assert moved == USED + (end - 128) == 5160
    assert host == 1010 + 1000


def test_three_host_frames_one_run(lib):
    frames = [frame(HOST, 0, 8000, 1010), frame(HOST, 1072, 4000, 505), frame(HOST, 1648, 800, 101)]
    rows, _, _, moved, host = plan(lib, frames)
    end2 = 1648 + 100 + 64
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, end2, 0, 3)]
    assert moved == USED + 1812
    assert host == (1010 + 1000) + (505 + 500) + (101 + 100)


def test_host_staging_host_in_batch_order(lib):
    frames = [frame(HOST, 0, 8000, 1010), frame(STAGED, 1072, 4800, 600, raw_off=32), frame(HOST, 1744, 800, 101)]
    rows, _, pull, moved, host = plan(lib, frames)
    assert not pull
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, 1064, 0, 1),
                    (RAW_STAGED, 32, BASE + 1072, 600, 1, 2), (DATA, BASE + 1744, BASE + 1744, 164, 2, 3)]
    assert moved == USED + 1064 + 600 + 164
    assert host == 2010 + 2 * 600 + 201


# A and B mirrored (the same distance in the raw area as in the caller's memory, B above A); C at
# another distance; D at C's distance but below it
H = frame(HOST, 0, 8000, 1010)
A = frame(CALLER, 1072, 2400, 300, raw_off=16, raw_src=SRC)
B = frame(CALLER, 1440, 1600, 200, raw_off=516, raw_src=SRC + 500)
C = frame(CALLER, 1712, 1200, 150, raw_off=2000, raw_src=SRC + 2000)
D = frame(CALLER, 1936, 800, 100, raw_off=1000, raw_src=SRC + 1000)


def _caller_rows(a, c):
    """With A at frame a and C at frame c: A and B as one span (B's distance + its length), C, D."""
    return [(RAW_CALLER, 16, SRC, 500 + 200, a, a + 2), (RAW_CALLER, 2000, SRC + 2000, 150, c, c + 1),
            (RAW_CALLER, 1000, SRC + 1000, 100, c + 1, c + 2)]


def test_caller_pinned_spans_come_last(lib):
    rows, _, _, moved, host = plan(lib, [H, A, B, C, D])
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, 1064, 0, 1)] + _caller_rows(1, 3)
    assert moved == USED + 1064 + 700 + 150 + 100       # the merged span with its gap
    assert host == 2010                                  # the host never touches a caller-pinned scan
    # the host frame between them: its copy still goes first, every caller span after it
    rows, _, _, moved2, host2 = plan(lib, [A, B, H, C, D])
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, 1064, 2, 3)] + _caller_rows(0, 3)
    assert (moved2, host2) == (moved, host)


@pytest.mark.parametrize("more, end", [((176, 1600), 176 + 200 + 64), ((16, 80), 0 + 100 + 64)])
def test_further_scan(lib, more, end):
    rows, _, _, moved, host = plan(lib, [frame(HOST, 0, 800, 350, more=more)])
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, end, 0, 1)]
    assert moved == USED + end
    assert host == 350 + 100 + more[1] // 8


def test_latency_one_host_frame_is_pulled(lib):
    f = [frame(HOST, 0, 80000, 10100)]
    length = 10000 + 64
    rows, segs, pull, moved, host = plan(lib, f, latency=True)
    assert pull and rows == []
    assert segs == [(0, USED // 16), (BASE // 16, -(-length // 16))] == [(0, 256), (4096, 629)]
    assert moved == USED + length and host == 10100 + 10000
    rows, segs, pull, moved2, _ = plan(lib, f, latency=True, prepulled=4096)
    assert pull and rows == []
    assert segs == [(0, 256), (4096 + 256, 629 - 256)]
    assert moved2 == moved                               # the run in full, though part went early


def test_latency_with_a_device_destuffed_frame_is_not_pulled(lib):
    frames = [frame(HOST, 0, 8000, 1010), frame(STAGED, 1072, 4800, 600, raw_off=32)]
    rows, segs, pull, _, _ = plan(lib, frames, latency=True)
    assert not pull and segs == []
    assert rows == [(HDR, 0, 0, USED, 0, 0), (DATA, BASE, BASE, 1064, 0, 1), (RAW_STAGED, 32, BASE + 1072, 600, 1, 2)]


def test_latency_five_host_frames_two_segments(lib):
    """Consecutive host-destuffed frames always merge, so a pulled batch has one
    data run: two of the pull kernel's four segments, however many frames."""
    frames = [frame(HOST, 1072 * i, 8000, 1010) for i in range(5)]
    rows, segs, pull, moved, host = plan(lib, frames, latency=True)
    end = 4 * 1072 + 1000 + 64
    assert pull and rows == []
    assert segs == [(0, 256), (4096, -(-end // 16))]
    assert moved == USED + end and host == 5 * 2010
