"""evf_store_segments_at (csrc/evf_eval_log.hip) through the C ABI: up to 32 segments copied into the row of a result log that a
device word names -- how a replayed evaluation step leaves its metrics without a host read.  The log is filled with a NaN-pattern
canary and compared as int32 words with what is expected, so every word outside the written row is a guard."""

import ctypes

import pytest
import torch

from event_flow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
ROW_FLOATS, NROWS = 300, 4
CANARY = 0x7FC0BEEF  # a quiet NaN with a payload


def fresh_log():
    words = torch.full(((NROWS + 2) * ROW_FLOATS,), CANARY, dtype=torch.int32, device=DEV)  # a guard row on either side
    return words, words[ROW_FLOATS:(NROWS + 1) * ROW_FLOATS].view(torch.float32)


def sources(lengths, seed=0):
    """One float32 source per length, cut at odd word offsets out of one arena (4-byte alignment is all the kernel may assume)."""
    g = torch.Generator().manual_seed(seed)
    arena = torch.rand(sum(lengths) + 4 * len(lengths) + 8, generator=g, dtype=torch.float32).to(DEV)
    out, at = [], 1
    for n in lengths:
        out.append(arena[at:at + max(n, 1)])  # (a segment of no floats still names memory: an empty tensor's pointer is NULL)
        at += max(n, 1) + 3
    return arena, out


def layout(lengths):
    """Offsets of the segments in the row: packed from float 2 on with a one-float gap, the last one ending at the row's end."""
    off, at = [], 2
    for n in lengths:
        off.append(at)
        at += n + 1
    assert at - 1 <= ROW_FLOATS
    off[-1] = ROW_FLOATS - lengths[-1]
    assert len(lengths) < 2 or off[-1] >= off[-2] + lengths[-2]
    return off


def arrays(src, off, lens):
    return ((ctypes.c_void_p * 32)(*[s.data_ptr() for s in src]), (ctypes.c_int * 32)(*off), (ctypes.c_int * 32)(*lens))


def store(row, src, off, lens, log):
    r = torch.tensor([row], dtype=torch.int64, device=DEV)
    rc = _lib.raw("evf_store_segments_at", r.data_ptr(), NROWS, log.data_ptr(), ROW_FLOATS, *arrays(src, off, lens), len(src))
    torch.cuda.synchronize()
    return rc


def expected(row, src, off, lens):
    words, log = fresh_log()
    for s, o, n in zip(src, off, lens):
        log[row * ROW_FLOATS + o:row * ROW_FLOATS + o + n] = s[:n]
    return words


CASES = {"four": [1, 0, 63, 64], "one": [257], "one-float": [1], "empty": [0],
         "thirty-two": [(5 * k) % 9 for k in range(31)] + [64]}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("row", [0, 3])
def test_segments_land_in_the_named_row(case, row):
    lens = CASES[case]
    _arena, src = sources(lens)
    off = layout(lens)
    words, log = fresh_log()
    assert store(row, src, off, lens, log) == 0
    want = expected(row, src, off, lens)
    bad = torch.nonzero(words != want).flatten()
    assert bad.numel() == 0, f"{bad.numel()} words differ, first at {int(bad[0])} (row {row}, offsets {off[:8]})"
    if sum(lens):
        assert not torch.equal(words, fresh_log()[0])


def test_257_floats_next_to_the_small_segments():
    """1, 0, 63, 64 and 257 floats do not fit one row of 300 together: the 257 with the 1 and the 0."""
    lens = [1, 0, 257]
    _arena, src = sources(lens, seed=3)
    off = layout(lens)
    for row in (0, 3):
        words, log = fresh_log()
        assert store(row, src, off, lens, log) == 0
        assert torch.equal(words, expected(row, src, off, lens))


@pytest.mark.parametrize("row", [-1, 4, 2 ** 40, -2 ** 40])
def test_a_row_outside_the_log_writes_nothing(row):
    lens = CASES["four"]
    _arena, src = sources(lens)
    words, log = fresh_log()
    assert store(row, src, layout(lens), lens, log) == 0
    assert torch.equal(words, fresh_log()[0])


def test_invalid_arguments():
    lens = [5, 7]
    _arena, src = sources(lens)
    words, log = fresh_log()
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    ok = arrays(src, [0, 10], lens)

    def call(r=row.data_ptr(), lg=log.data_ptr(), a=ok, nseg=2, row_floats=ROW_FLOATS):
        return _lib.raw("evf_store_segments_at", r, NROWS, lg, row_floats, a[0], a[1], a[2], nseg)

    assert call(r=None) == EINVAL and call(lg=None) == EINVAL
    assert call(a=(None, ok[1], ok[2])) == EINVAL and call(a=(ok[0], None, ok[2])) == EINVAL and call(a=(ok[0], ok[1], None)) == EINVAL
    assert call(nseg=0) == EINVAL and call(nseg=-1) == EINVAL and call(nseg=33) == EINVAL
    assert call(a=arrays(src, [0, 10], [5, -1])) == EINVAL and call(a=arrays(src, [0, -1], lens)) == EINVAL
    assert call(a=arrays(src, [0, ROW_FLOATS - 6], lens)) == EINVAL       # the second segment ends one float behind the row
    assert call(a=arrays(src, [0, ROW_FLOATS], [5, 1])) == EINVAL
    assert call(a=arrays(src, [0, 2 ** 31 - 4], [5, 7])) == EINVAL          # offset + n beyond int32: no wrap-around
    assert call(row_floats=16) == EINVAL                                     # ... against the row length given
    null = ((ctypes.c_void_p * 32)(src[0].data_ptr(), None), ok[1], ok[2])
    assert call(a=null) == EINVAL
    assert call(a=(null[0], ok[1], (ctypes.c_int * 32)(5, 0))) == EINVAL     # a NULL source of no floats, too
    odd = ((ctypes.c_void_p * 32)(src[0].data_ptr(), src[1].data_ptr() + 2), ok[1], ok[2])
    assert call(a=odd) == EINVAL                                             # a source that is not 4-byte aligned
    torch.cuda.synchronize()
    assert torch.equal(words, fresh_log()[0])                                # nothing was launched
    assert call(a=arrays(src, [0, ROW_FLOATS - 7], lens)) == 0               # the second segment ends with the row
    assert call(a=arrays(src, [0, ROW_FLOATS], [5, 0])) == 0                 # n == 0 at the row's end
    torch.cuda.synchronize()
    assert torch.equal(words, expected(0, src, [0, ROW_FLOATS - 7], lens))


def test_captured_call_reads_the_row_at_replay():
    """The call in a hipGraph, replayed twice with the row word rewritten in between by a device copy: each replay fills its own
    row from what the sources hold then."""
    lens = CASES["four"]
    arena, src = sources(lens)
    off = layout(lens)
    words, log = fresh_log()
    row = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    rows = torch.tensor([2, 0], dtype=torch.int64, device=DEV)
    a = arrays(src, off, lens)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _lib.call("evf_store_segments_at", row.data_ptr(), NROWS, log.data_ptr(), ROW_FLOATS, *a, len(src))
    torch.cuda.synchronize()
    assert torch.equal(words, fresh_log()[0]), "the capture itself wrote"
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(words, fresh_log()[0]), "replay with row -1 wrote"
    row.copy_(rows[0:1])
    g.replay()
    torch.cuda.synchronize()
    want = expected(2, src, off, lens)
    assert torch.equal(words, want)
    arena.mul_(2.0)
    row.copy_(rows[1:2])
    g.replay()
    torch.cuda.synchronize()
    want_log = want[ROW_FLOATS:(NROWS + 1) * ROW_FLOATS].view(torch.float32)
    for s, o, n in zip(src, off, lens):
        want_log[o:o + n] = s[:n]
    assert torch.equal(words, want)
