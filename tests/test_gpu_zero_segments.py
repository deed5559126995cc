"""evf_zero_segments_if (csrc/evf_resident.hip) through the C ABI: the conditional zero-fill of up to 32 segments that resets the
recurrent state inside a replayed training step.  All segments of a call lie in ONE int32 arena filled with a canary pattern, at
least four canary words between neighbours, and the whole arena is compared with what is expected: every byte outside the
segments is a guard."""

import ctypes

import numpy as np
import pytest
import torch

from event_flow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
SWEEP = 3 * 2 ** 20 + 4  # more than the 2 MiB one sweep of the grid covers, + a one-word tail


def layout(segments):
    """segments: (start misalignment mod 16 in bytes, length in bytes) -> (arena words, [(first word, words)])."""
    at, out = 8, []
    for mis, nbytes in segments:
        at = (at + 3) // 4 * 4 + mis // 4  # the arena is 16-byte aligned: word index mod 4 is the misalignment
        out.append((at, nbytes // 4))
        at += nbytes // 4 + 4
    return at + 8, out


def arena(words):
    return (torch.arange(words, dtype=torch.int32, device=DEV) * 7919) | 1  # (no word of the canary pattern is zero)


def run(flag, segments, base=None):
    """One call on a fresh arena -> (status, arena after, arena before, word ranges)."""
    words, where = layout(segments)
    a = arena(words)
    before = a.clone()
    assert a.data_ptr() % 16 == 0
    n = len(where)
    dst = (ctypes.c_void_p * 32)(*[a.data_ptr() + 4 * w for w, _ in where])
    size = (ctypes.c_int64 * 32)(*[4 * k for _, k in where])
    f = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=DEV)
    rc = _lib.raw("evf_zero_segments_if", None if f is None else f.data_ptr(), dst, size, n)
    torch.cuda.synchronize()
    return rc, a, before, where


def expected(before, where):
    want = before.clone()
    for w, k in where:
        want[w:w + k] = 0
    return want


# 4 bytes; 16k + 4, + 8, + 12; a start 4 (and 8, 12) mod 16; 0 bytes; larger than one grid sweep
SEVEN = [(0, 4), (0, 16 * 9 + 4), (0, 16 * 5 + 8), (4, 16 * 3 + 12), (12, 0), (8, 16 * 2), (4, SWEEP)]
CASES = {"seven": SEVEN, "one": [(4, 16 * 70 + 8)],
         "thirty-two": [((4 * k) % 16, 4 * ((37 * k) % 23) + (4096 if k == 30 else 0)) for k in range(32)]}


@pytest.mark.parametrize("case", sorted(CASES))
def test_zero_fill_follows_the_flag(case):
    segs = CASES[case]
    rc, a, before, where = run(0, segs)
    assert rc == 0 and torch.equal(a, before), "flag 0 wrote something"
    for flag in (1, -1, None):
        rc, a, before, where = run(flag, segs)
        assert rc == 0
        want = expected(before, where)
        bad = torch.nonzero(a != want).flatten()
        assert bad.numel() == 0, f"flag {flag}: {bad.numel()} words differ, first at word {int(bad[0])} (segments {where[:8]})"


def test_invalid_arguments():
    a = arena(64)
    ok_dst, ok_size = (ctypes.c_void_p * 32)(a.data_ptr() + 16), (ctypes.c_int64 * 32)(16)
    call = lambda *args: _lib.raw("evf_zero_segments_if", None, *args)  # noqa: E731
    assert call(ok_dst, ok_size, 1) == 0
    assert call(None, ok_size, 1) == EINVAL and call(ok_dst, None, 1) == EINVAL
    assert call(ok_dst, ok_size, 0) == EINVAL and call(ok_dst, ok_size, -1) == EINVAL and call(ok_dst, ok_size, 33) == EINVAL
    assert call((ctypes.c_void_p * 32)(None), ok_size, 1) == EINVAL                      # a NULL segment
    assert call((ctypes.c_void_p * 32)(None), (ctypes.c_int64 * 32)(0), 1) == EINVAL     # ... of no bytes, too
    assert call((ctypes.c_void_p * 32)(a.data_ptr() + 18), ok_size, 1) == EINVAL         # misaligned
    assert call(ok_dst, (ctypes.c_int64 * 32)(-4), 1) == EINVAL and call(ok_dst, (ctypes.c_int64 * 32)(6), 1) == EINVAL
    two = (ctypes.c_void_p * 32)(a.data_ptr() + 16, a.data_ptr() + 130)                  # the second of two segments
    assert call(two, (ctypes.c_int64 * 32)(16, 16), 2) == EINVAL
    torch.cuda.synchronize()
    want = arena(64)
    want[4:8] = 0
    assert torch.equal(a, want)  # only the one valid call wrote


def test_captured_call_reads_the_flag_at_replay():
    """The call in a hipGraph, replayed with the flag tensor rewritten in between (0, then 1), against the eager call."""
    words, where = layout(SEVEN)
    a = arena(words)
    before = a.clone()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    dst = (ctypes.c_void_p * 32)(*[a.data_ptr() + 4 * w for w, _ in where])
    size = (ctypes.c_int64 * 32)(*[4 * k for _, k in where])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _lib.call("evf_zero_segments_if", flag.data_ptr(), dst, size, len(where))
    torch.cuda.synchronize()
    assert torch.equal(a, before), "the capture itself wrote"
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, before), "replay with flag 0 wrote"
    flag.fill_(1)
    g.replay()
    torch.cuda.synchronize()
    _rc, eager, _b, _w = run(1, SEVEN)
    assert torch.equal(a, expected(before, where)) and torch.equal(a, eager)
