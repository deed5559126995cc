"""Rig streaming on the MI355X (event_flow_amd/rig_stream.py, csrc/evf_stream.hip, infer_flow.py --window-dt): evf_rings_append
against numpy rings across the wrap, evf_rings_cut_ragged against evf_seq_cut_ragged on the linear arena of the same events bit
for bit, their guards and captured replays; `RigStream` fed sequence files in several chunkings against the eager evaluation loop on
`ResidentEvalLoader` in `time` mode (B = 1 and B = 2), window by window with torch.equal; overflow, replay, reset, the watermark,
the result ring, slot independence; the driver in a fresh process."""

import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from test_gpu_eval_graphed import _initial
from test_gpu_stream import CANARY, _events, _guarded, _model, _ring_of, det_on  # noqa: F401 (det_on: a fixture)
from test_host_eval_steps import H, W
from test_host_loader import _cfg

from event_flow_amd import _lib
from event_flow_amd.dataloader.h5 import write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader
from event_flow_amd.rig_stream import RigStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPAD = 300           # max_events: deliberately no multiple of the 256-thread block
R = 2 * NPAD + 37    # every ring wraps several times
T0, DT, NWIN = 100.0, 0.1, 20
LAST = T0 + 2.03     # the files' last timestamp: on no border
EMPTY = (1, 7)       # (camera, window) with 6 events: cut as empty for that camera


def _staged_bytes(heads, cols):
    """The staged buffer of one push: int64 head [B] | int64 offsets [B + 1] | ts | xs | ys | ps of all cameras in camera order."""
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cols])]).astype(np.int64)
    parts = [np.asarray(heads, dtype=np.int64).view(np.uint8), off.view(np.uint8)]
    for k in (2, 0, 1, 3):
        parts += [np.ascontiguousarray(c[k]).view(np.uint8) for c in cols]
    return np.concatenate(parts)


def _rings_guarded(B, fills):
    """The four [B, R] columns with CANARY elements in front of and behind each -> [(whole tensor, pointer of the column)]."""
    return [_guarded(dt, B * R, f) for dt, f in zip((torch.uint16, torch.uint16, torch.float64, torch.uint8), fills)]


# ------------------------------------------------------------------ evf_rings_append
def test_append_to_three_rings_equals_numpy_rings():
    B = 3
    cams = [_events(3 * R, 40 + b) for b in range(B)]
    fills = (0x7A7A, 0x7A7A, -77.25, 0x7A)
    dev = _rings_guarded(B, fills)
    ref = [np.full((B, R), f, dtype=c.dtype) for c, f in zip(cams[0], fills)]
    stage = torch.zeros(8 * (2 * B + 1) + 13 * B * R + 16, dtype=torch.uint8, device=DEV)
    at = stage.data_ptr()
    heads = [0, 0, 0]

    def send(heads_sent, cols):
        host = _staged_bytes(heads_sent, cols)
        stage.fill_(0xEE)
        stage[:len(host)].copy_(torch.from_numpy(host))
        return len(host)

    def append(cols, most=None):
        counts = [len(c[0]) for c in cols]
        _lib.call("evf_rings_append", at, B, sum(counts), max(counts) if most is None else most, *(p for _t, p in dev), R)

    def check(what):
        for (t, _p), r, f, name in zip(dev, ref, fills, ("xs", "ys", "ts", "ps")):
            got = t.cpu().numpy().view(r.dtype)
            assert np.array_equal(got[CANARY:-CANARY].reshape(B, R), r), (name, what)  # (a ring's neighbours are its canaries)
            assert np.all(got[:CANARY] == r.dtype.type(f)) and np.all(got[-CANARY:] == r.dtype.type(f)), ("canary", name, what)

    # per-camera counts {0, 1, 257} in every order, then whole rings: every ring wraps
    for counts in ((0, 1, 257), (257, 0, 1), (1, 257, 0), (R, 257, R), (257, 1, 0), (0, 257, 1), (1, 0, 257), (257, R, 1)):
        cols = [tuple(c[h:h + n] for c in cam) for cam, h, n in zip(cams, heads, counts)]
        used = send(heads, cols)
        append(cols)
        for b, (h, n) in enumerate(zip(heads, counts)):
            ids = np.arange(h, h + n)
            for r, c in zip(ref, cams[b]):
                r[b, ids % R] = c[ids]
        heads = [h + n for h, n in zip(heads, counts)]
        check(counts)
        assert np.all(stage.cpu().numpy()[used:] == 0xEE)
    assert min(heads) > R  # every ring wrapped
    # a negative head word writes nothing for that camera, the others are written
    counts = (5, 257, 9)
    cols = [tuple(c[h:h + n] for c in cam) for cam, h, n in zip(cams, heads, counts)]
    send([heads[0], -1, heads[2]], cols)
    append(cols)
    for b in (0, 2):
        ids = np.arange(heads[b], heads[b] + counts[b])
        for r, c in zip(ref, cams[b]):
            r[b, ids % R] = c[ids]
    check("negative head")
    # an offset table that does not ascend from 0 to n, or gives a camera more than R events, writes nothing at all
    n = sum(counts)
    for off in ([0, 262, 5, n], [1, 5, 262, n], [0, 5, 262, n - 1], [0, 5, 262, n + 1], [-1, 5, 262, n], [0, -5, 262, n]):
        send(heads, cols)
        stage[8 * B:8 * (2 * B + 1)].copy_(torch.from_numpy(np.array(off, dtype=np.int64).view(np.uint8)))
        append(cols)
        check(off)
    wide = [tuple(c[:m] for c in cams[0]) for m in (R, R, 2)]  # the table says (R + 1, R - 1, 2)
    send(heads, wide)
    stage[8 * B:8 * (2 * B + 1)].copy_(torch.from_numpy(np.array([0, R + 1, 2 * R, 2 * R + 2], dtype=np.int64).view(np.uint8)))
    append(wide)
    check("a camera with more than R events")
    send(heads, [tuple(c[:0] for c in cam) for cam in cams])
    append([tuple(c[:0] for c in cam) for cam in cams])  # no events launch nothing
    check("no events")

    # every EVF_EINVAL case
    ptrs = [p for _t, p in dev]
    ok = [at, B, 271, 257] + ptrs + [R]  # (the staged push of 5 + 257 + 9 events)
    send(heads, cols)
    assert _lib.raw("evf_rings_append", *ok) == 0
    for i, bad in ((0, None), (4, None), (5, None), (6, None), (7, None), (1, 0), (1, -1), (1, 17), (2, -1), (3, -1), (3, 272), (3, R + 1),
                   (3, 87), (8, 0), (8, -5), (8, 256), (0, at + 4), (6, ptrs[2] + 4), (4, ptrs[0] + 1), (5, ptrs[1] + 1)):
        args = list(ok)
        args[i] = bad
        assert _lib.raw("evf_rings_append", *args) == -22, ("evf_rings_append", i, bad)
    torch.cuda.synchronize()


def test_append_captured_and_replayed():
    B = 3
    cams = [_events(3 * R, 50 + b) for b in range(B)]
    start = [R - 20, 2 * R - 100, 5]  # the rings' heads: across the end | across it on the second replay | far from it
    rings = [torch.from_numpy(np.stack([_ring_of(cam, s, R)[k] for cam, s in zip(cams, start)])).to(DEV) for k in range(4)]
    eager = [c.clone() for c in rings]
    stage = torch.zeros(8 * (2 * B + 1) + 13 * B * R, dtype=torch.uint8, device=DEV)
    at = stage.data_ptr()
    n, most = 258, 257

    def load(heads, counts):
        cols = [tuple(c[h:h + m] for c in cam) for cam, h, m in zip(cams, heads, counts)]
        host = _staged_bytes(heads, cols)
        stage[:len(host)].copy_(torch.from_numpy(host))

    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    heads = list(start)
    load(heads, (0, 1, 257))
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        _lib.call("evf_rings_append", at, B, n, most, *(_lib.ptr(c) for c in rings), R)
    for counts in ((0, 1, 257), (257, 0, 1), (100, 100, 58)):  # the same launch, another table and chunk
        load(heads, counts)
        _lib.call("evf_rings_append", at, B, n, most, *(_lib.ptr(c) for c in eager), R)
        graph.replay()
        torch.cuda.synchronize()
        heads = [h + m for h, m in zip(heads, counts)]
        for k in range(4):
            want = np.stack([_ring_of(cam, h, R)[k] for cam, h in zip(cams, heads)])
            assert torch.equal(rings[k], eager[k]) and np.array_equal(rings[k].cpu().numpy().view(want.dtype), want), (counts, k)


# ------------------------------------------------------------------ evf_rings_cut_ragged
APPENDED = 2230  # a ring holds its camera's events [APPENDED - R, APPENDED) = [1593, 2230); event 3 R = 1911 sits in slot 0
STARTS = {"before": lambda c: 3 * R - c - 3, "across": lambda c: 3 * R - c // 2, "after": lambda c: 3 * R + 5,
          "oldest": lambda c: APPENDED - R, "newest": lambda c: APPENDED - c}
COUNTS = (0, 11, 255, 256, 257, 300)


@pytest.fixture(scope="module")
def three_cameras():
    cams = [_events(4 * R, 60 + b) for b in range(3)]
    lin = [torch.from_numpy(np.concatenate([cam[k] for cam in cams])).to(DEV) for k in range(4)]
    rings = [torch.from_numpy(np.stack([_ring_of(cam, APPENDED + 7 * b, R)[k] for b, cam in enumerate(cams)])).to(DEV) for k in range(4)]
    return cams, lin, rings


def _seq_cut_ragged(lin, first, count, flags, npad):
    J = len(first)
    ev = torch.full((J, npad, 4), 9.0, dtype=torch.float32, device=DEV)
    dt = torch.full((J,), 9.0, dtype=torch.float64, device=DEV)
    f, c, fl = (torch.tensor(v, dtype=d, device=DEV) for v, d in ((first, torch.int64), (count, torch.int32), (flags, torch.int32)))
    _lib.call("evf_seq_cut_ragged", *(_lib.ptr(t) for t in lin), lin[0].numel(), _lib.ptr(f), _lib.ptr(c), _lib.ptr(fl), J, npad, H, W,
              _lib.ptr(ev), _lib.ptr(dt))
    torch.cuda.synchronize()  # (the table tensors live until the launch has read them)
    return ev, dt


def _table(first, appended, count, flags):
    B = len(first)
    tab = np.zeros(2 * B + B, dtype=np.int64)
    tab[:B], tab[B:2 * B] = first, appended
    aux = tab[2 * B:].view(np.int32)
    aux[:B], aux[B:] = count, flags
    return tab


def _rings_cut(rings, tab_dev, B, npad, ev_ptr, dt_ptr, cap=R, call=None):
    at = tab_dev.data_ptr()
    (call or _lib.call)("evf_rings_cut_ragged", *(_lib.ptr(t) for t in rings), cap, at, at + 8 * B, at + 16 * B, at + 20 * B, B, npad, H, W,
                        ev_ptr, dt_ptr)


@pytest.mark.parametrize("start", sorted(STARTS))
def test_cut_equals_seq_cut_ragged_on_the_linear_arena(three_cameras, start):
    cams, lin, rings = three_cameras
    B, n_lin = 3, len(cams[0][0])
    appended = [APPENDED + 7 * b for b in range(B)]
    live = 0
    for shift in range(len(COUNTS)):  # three different counts a launch, every count in every ring
        count = [COUNTS[(shift + 2 * b) % len(COUNTS)] for b in range(B)]
        first = [STARTS[start](c) + 7 * b for b, c in enumerate(count)]
        flags = [(shift + 3 * b) % 8 for b in range(B)]
        for f, c, a in zip(first, count, appended):
            assert a - R <= f and f + c <= a
        tab = torch.from_numpy(_table(first, appended, count, flags)).to(DEV)
        ev = torch.full((B, NPAD, 4), 9.0, dtype=torch.float32, device=DEV)
        dt = torch.full((B,), 9.0, dtype=torch.float64, device=DEV)
        _rings_cut(rings, tab, B, NPAD, _lib.ptr(ev), _lib.ptr(dt))
        want_ev, want_dt = _seq_cut_ragged(lin, [b * n_lin + f for b, f in enumerate(first)], count, flags, NPAD)
        assert torch.equal(ev.view(torch.int32), want_ev.view(torch.int32)), (start, count)  # bit for bit
        assert torch.equal(dt.view(torch.int64), want_dt.view(torch.int64)), (start, count)
        for b, c in enumerate(count):
            assert not ev[b, c:].any() and (c == 0 or not torch.any(ev[b, :c, 3] == 0)) and (float(dt[b]) > 0) == (c > 0)
            live += c
    assert live == 3 * sum(COUNTS)


def test_cut_refused_jobs_einval_and_captured_replay(three_cameras):
    cams, lin, rings = three_cameras
    B, n_lin = 3, len(cams[0][0])
    appended = [APPENDED + 7 * b for b in range(B)]
    good_first, good_count = [1700, 1900, 2000], [257, 300, 11]
    # -- the kernel's own guard: one refused job next to two fine ones, in every ring
    refused = {"count = 0": (1700, 0, NPAD), "count < 0": (1700, -3, NPAD), "count > Npad": (1700, NPAD + 1, NPAD),
               "count > R": (APPENDED - R, R + 1, R + 5), "first < appended - R": (APPENDED - R - 1, 50, NPAD),
               "first + count > appended": (APPENDED - 49, 50, NPAD), "first < 0": (-1, 50, NPAD), "first far below": (-(2 ** 40), 50, NPAD),
               "first = appended": (APPENDED, 1, NPAD)}
    for what, (f, c, npad) in refused.items():
        for bad in range(B):
            first, count = list(good_first), list(good_count)
            first[bad], count[bad] = f + 7 * bad, c
            flags = [3, 5, 6]
            tab = torch.from_numpy(_table(first, appended, count, flags)).to(DEV)
            ev, ev_ptr = _guarded(torch.float32, B * npad * 4, 9.0)
            dt, dt_ptr = _guarded(torch.float64, B, 9.0)
            assert ev_ptr % 16 == 0
            _rings_cut(rings, tab, B, npad, ev_ptr, dt_ptr)
            rows = ev[CANARY:-CANARY].view(B, npad, 4)
            keep = [b for b in range(B) if b != bad]
            want_ev, want_dt = _seq_cut_ragged(lin, [b * n_lin + first[b] for b in keep], [count[b] for b in keep],
                                               [flags[b] for b in keep], npad)
            assert not rows[bad].any() and float(dt[CANARY + bad]) == 0.0, (what, bad)  # all-zero rows and dt = 0
            for j, b in enumerate(keep):
                assert torch.equal(rows[b].view(torch.int32), want_ev[j].view(torch.int32)), (what, bad, b)
                assert float(dt[CANARY + b]) == float(want_dt[j]) > 0
            for t in (ev, dt):  # ... and nothing else
                assert bool((t[:CANARY] == 9.0).all()) and bool((t[-CANARY:] == 9.0).all()), (what, bad)

    # -- every EVF_EINVAL case
    tab = torch.from_numpy(_table(good_first, appended, good_count, [0, 0, 0])).to(DEV)
    out_ev = torch.zeros((B, NPAD, 4), dtype=torch.float32, device=DEV)
    out_dt = torch.zeros(B, dtype=torch.float64, device=DEV)
    at = tab.data_ptr()
    ok = [_lib.ptr(t) for t in rings] + [R, at, at + 8 * B, at + 16 * B, at + 20 * B, B, NPAD, H, W, _lib.ptr(out_ev), _lib.ptr(out_dt)]
    assert _lib.raw("evf_rings_cut_ragged", *ok) == 0
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (7, None), (8, None), (13, None), (14, None), (4, 0),
                   (4, -1), (9, 0), (9, -1), (9, 17), (10, 0), (10, -3), (11, 0), (12, 0), (5, at + 4), (6, at + 8 * B + 4), (7, at + 16 * B + 2),
                   (8, at + 20 * B + 2), (2, ok[2] + 4), (0, ok[0] + 1), (1, ok[1] + 1), (13, ok[13] + 4), (14, ok[14] + 4)):
        args = list(ok)
        args[i] = bad
        assert _lib.raw("evf_rings_cut_ragged", *args) == -22, ("evf_rings_cut_ragged", i, bad)

    # -- one captured call, replayed with a rewritten table
    ev_r, dt_r = torch.zeros_like(out_ev), torch.zeros_like(out_dt)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        _rings_cut(rings, tab, B, NPAD, _lib.ptr(ev_r), _lib.ptr(dt_r))
    for first, count, flags in ((good_first, good_count, [0, 0, 0]), ([1911, 1750, 2230], [300, 0, 14], [1, 2, 4]),
                                ([1600, 1800, 1650], [11, 256, 255], [7, 0, 3])):
        tab.copy_(torch.from_numpy(_table(first, appended, count, flags)))
        graph.replay()
        torch.cuda.synchronize()
        want_ev, want_dt = _seq_cut_ragged(lin, [b * n_lin + f for b, f in enumerate(first)], count, flags, NPAD)
        assert torch.equal(ev_r.view(torch.int32), want_ev.view(torch.int32)) and torch.equal(dt_r, want_dt), (first, count)
        assert float(ev_r.abs().max()) > 0


# ------------------------------------------------------------------ RigStream against the loader
def _camera(b):
    """Camera b's recording: NWIN windows of 100 .. 189 events (6 in the EMPTY one), distinct timestamps, the first exactly T0,
    a few behind the last border up to exactly LAST -> (xs, ys, ts, ps) as a file holds them."""
    rng = np.random.Generator(np.random.PCG64(70 + b))
    ts, row = [], 0.0
    for k in range(NWIN):
        n = 6 if (b, k) == EMPTY else int(rng.integers(100, 190))
        ts.append(row + T0 + (np.arange(n) + 0.25 + 0.5 * rng.random(n)) / n * DT * 0.96)
        row += DT
    ts.append(row + T0 + 0.001 + np.sort(rng.random(14)) * 0.025)
    ts = np.concatenate(ts + [[LAST]])
    ts[0] = T0
    assert np.all(np.diff(ts) > 0)
    n = len(ts)
    return rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), ts, rng.integers(0, 2, n).astype(np.uint8)


def _files(path, cams):
    os.makedirs(path, exist_ok=True)
    for b, (xs, ys, ts, ps) in enumerate(cams):
        write_npz_sequence(os.path.join(str(path), f"s{b}.npz"), xs, ys, ts, ps)
    return [os.path.join(str(path), f"s{b}.npz") for b in range(len(cams))]


def _loader_flows(path, B, model, hot, dt=DT):
    """eval_flow.py's eager loop on ResidentEvalLoader in `time` mode up to the first restart -> per window (flow [B,2,H,W],
    event mask [B,H,W])."""
    ld = ResidentEvalLoader(_cfg(path, "time", dt, B, (H, W), (), hot=hot), 2)
    out = []
    with torch.no_grad():
        for i, inputs in enumerate(ld):
            if ld.new_seq:
                if i > 0:
                    break
                ld.new_seq = False
                model.reset_states()
            if ld.pass_done:
                break
            x = model(inputs["event_voxel"], inputs["event_cnt"])
            out.append((x["flow"][-1].clone(), inputs["event_mask"][:, 0].clone()))
    return out


def _config(hot):
    return _cfg("unused", "time", DT, 1, (H, W), (), hot=hot)


def _feed(rig, cams, cut, advance=None):
    """Push `cams` in pushes of cut(rig, at) events per camera -> per window (flow, mask, result) cloned call by call."""
    out, at = [], [0] * len(cams)
    while any(a < len(c[0]) for a, c in zip(at, cams)):
        take = [min(int(n), len(c[0]) - a) for n, a, c in zip(cut(rig, at), at, cams)]
        for r in rig.push([tuple(col[a:a + n] for col in c) for c, a, n in zip(cams, at, take)]):
            out.append((r.flow.clone(), r.event_mask.clone(), r))
        at = [a + n for a, n in zip(at, take)]
    if advance is not None:
        for r in rig.advance(advance):
            out.append((r.flow.clone(), r.event_mask.clone(), r))
    return out


def _few(cams):
    """23 events a push, in the time order of all cameras."""
    cam_of = np.concatenate([np.full(len(c[2]), b) for b, c in enumerate(cams)])[np.argsort(np.concatenate([c[2] for c in cams]),
                                                                                              kind="stable")]
    return lambda rig, at: np.bincount(cam_of[sum(at):sum(at) + 23], minlength=len(cams))


def _by_time(cams, span, lag=0.0):
    """Push i: camera 0 up to T0 + (i + 1) span, the other cameras `lag` behind it."""
    calls = [0]

    def cut(rig, at):
        calls[0] += 1
        return [np.searchsorted(c[2], T0 + calls[0] * span - (lag if b else 0.0)) - a for b, (c, a) in enumerate(zip(cams, at))]

    return cut


CHUNKINGS = {"a few events": _few, "several windows": lambda cams: _by_time(cams, 2.2 * DT),
             "one camera ahead": lambda cams: _by_time(cams, 0.7 * DT, lag=0.7 * DT), "largest": lambda cams: lambda rig, at: rig.max_push}


def _against_the_loader(path, kind, hot, B):
    cams = [_camera(b) for b in range(B)]
    _files(path, cams)
    sd0 = _initial(kind)
    want = _loader_flows(path, B, _model(kind, sd0), hot)
    assert len(want) == NWIN and all(float(f.abs().max()) > 0 for f, _m in want)  # nonzero flow in every window
    assert len({float(f.abs().sum()) for f, _m in want}) == len(want)             # ... pairwise different
    if B > 1:
        assert not want[EMPTY[1]][1][EMPTY[0]].any() and all(m[0].any() for _f, m in want)  # an empty window in one camera only
    for label, chunks in CHUNKINGS.items():
        rig = RigStream(_model(kind, sd0), _config(hot), cameras=B, window_dt=DT, max_events=NPAD, capacity=R, slots=8, t0=T0)
        got = _feed(rig, cams, chunks(cams))
        torch.cuda.synchronize()
        assert len(got) == len(want) and rig.appended == [len(c[0]) for c in cams], label
        assert min(rig.appended) > 3 * R  # every ring wrapped several times
        for k, ((flow, mask, r), (wf, wm)) in enumerate(zip(got, want)):
            assert torch.equal(flow, wf), (label, "flow of window", k)
            assert torch.equal(mask, wm), (label, "event mask of window", k)
            assert r.index == k and r.dropped == [0] * B
            for b, c in enumerate(cams):
                lo, hi = np.searchsorted(c[2], [r.t_begin + T0, (r.t_begin + T0) + DT])
                assert (r.first[b], r.count[b]) == (lo, hi - lo if hi - lo > 10 else 0), (label, k, b)
        assert rig.stats["replayed"] == len(want) - 2 >= 2 and rig.stats["windows"] == len(want), (label, rig.stats)
        if B > 1:
            assert got[EMPTY[1]][2].count[EMPTY[0]] == 0
        assert rig.rings.copies == rig.stats["appends"] <= rig.stats["pushes"]  # one copy and one launch a push


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("kind", ["lif", "plif"])
def test_rig_equals_the_loader_deterministic(tmp_path, det_on, kind, hot, B):
    _against_the_loader(tmp_path, kind, hot, B)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind", ["lif", "plif"])
def test_rig_equals_the_loader_default_mode_count_input(tmp_path, kind, B):
    """The default (float-atomic) mode: the networks read the count encoding, whose sums of +-1 are exact in any order."""
    assert not _lib.deterministic()
    _against_the_loader(tmp_path, kind, True, B)


# ------------------------------------------------------------------ overflow, replay, reset, the watermark, the result ring
def _rig(sd0, B, **kw):
    kw = {**dict(cameras=B, window_dt=DT, max_events=NPAD, capacity=R, slots=8, t0=T0), **kw}
    return RigStream(_model("lif", sd0), _config(True), **kw)


def test_overflow_newest_equals_a_stream_without_the_oldest(det_on):
    xs, ys, ts, ps = _camera(0)
    rng = np.random.Generator(np.random.PCG64(81))
    n0 = int(np.searchsorted(ts, T0 + DT))
    m = NPAD + 40 - n0  # events added to window 0: it then holds max_events + 40
    extra = np.sort(T0 + 0.0001 + rng.random(m) * DT * 0.97)
    full = [np.concatenate([a[:n0], b, a[n0:]]) for a, b in ((xs, rng.integers(0, W, m).astype(np.uint16)),
                                                             (ys, rng.integers(0, H, m).astype(np.uint16)), (ts, extra),
                                                             (ps, rng.integers(0, 2, m).astype(np.uint8)))]
    order = np.argsort(full[2][:n0 + m], kind="stable")
    full = [np.concatenate([c[:n0 + m][order], c[n0 + m:]]) for c in full]
    assert np.searchsorted(full[2], T0 + DT) == NPAD + 40 and full[2][0] == T0
    sd0 = _initial("lif")
    upto = int(np.searchsorted(full[2], T0 + 5 * DT)) + 1  # five windows
    newest = _rig(sd0, 1, overflow="newest")
    got = _feed(newest, [tuple(c[:upto] for c in full)], lambda rig, at: [150])
    plain = _rig(sd0, 1)
    want = _feed(plain, [tuple(c[40:upto] for c in full)], lambda rig, at: [150])
    torch.cuda.synchronize()
    assert len(got) == len(want) == 5
    assert got[0][2].dropped == [40] and got[0][2].first == [40] and got[0][2].count == [NPAD] and want[0][2].count == [NPAD]
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) and float(g[0].abs().max()) > 0, k
        assert k == 0 or g[2].dropped == [0]
    # overflow="raise" refuses the same window before any copy or launch, the stream's state untouched
    strict = _rig(sd0, 1)
    strict.push([tuple(c[:200] for c in full)])
    state = (strict.plan.counters(), dict(strict.stats), strict.rings.copies)
    with pytest.raises(_lib.EvflowError, match="max_events = 300.*overflow='newest'"):
        strict.push([tuple(c[200:400] for c in full)])
    assert state == (strict.plan.counters(), dict(strict.stats), strict.rings.copies)


def test_replay_reset_watermark_result_ring_and_slot_independence(det_on):
    cams = [_camera(0), _camera(1)]
    sd0 = _initial("lif")

    def run(replay, twice=False):
        rig = _rig(sd0, 2, replay=replay)
        got = _feed(rig, cams, _by_time(cams, 2.2 * DT))
        if twice:
            rig.reset()
            assert rig.appended == [0, 0] and rig.plan.windows == 0 and rig.plan.row == 0.0
            got += _feed(rig, cams, _few(cams))
        torch.cuda.synchronize()
        return rig, got

    r1, g1 = run(True)
    r0, g0 = run(False)
    assert len(g1) == len(g0) == NWIN
    for k, (a, b) in enumerate(zip(g1, g0)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
    assert r0.stats["eager"] == NWIN and r0.stats["replayed"] == 0
    assert r1.stats["eager"] == 2 and r1.stats["replayed"] == NWIN - 2 and r1.stats["graph_a"] >= 1 and r1.stats["graph_b"] >= 1
    last = g1[-1][2]
    assert last.flow.shape == (2, 2, H, W) and last.event_mask.shape == (2, H, W)
    assert r1.model.mask and torch.equal(last.flow_masked, last.flow * last.event_mask[:, None]) and last.ready.query()
    # reset(): the same recording twice gives the first run's flows both times (the second time under the replayed zero-fill)
    r2, g2 = run(True, twice=True)
    assert len(g2) == 2 * NWIN and r2.stats["replayed_reset"] == 1
    for k in range(NWIN):
        for half in (g2[k], g2[NWIN + k]):
            assert torch.equal(half[0], g1[k][0]) and torch.equal(half[1], g1[k][1]), k
        assert g2[NWIN + k][2].index == k
    # advance(t): camera 1 falls silent behind window 2; the declaration completes the windows its silence held back
    rig = _rig(sd0, 2)
    cut0, cut1, stop = (int(np.searchsorted(c[2], T0 + k * DT)) for c, k in ((cams[0], 5), (cams[1], 3), (cams[0], 3)))
    quiet = tuple(c[:0] for c in cams[1])
    done = _feed(rig, [tuple(c[:stop + 1] for c in cams[0]), tuple(c[:cut1] for c in cams[1])], _by_time(cams, 0.9 * DT))
    assert [r.index for _f, _m, r in done] == [0, 1]  # (camera 1 has not passed window 2's closing border)
    assert rig.push([tuple(c[stop + 1:cut0] for c in cams[0]), quiet]) == []
    more = rig.advance(T0 + 5 * DT + 1e-6)
    assert [r.index for r in more] == [2, 3, 4] and [r.count[1] > 0 for r in more] == [True, False, False]
    assert all(r.count[0] > 10 for r in more) and rig.advance(T0 + 5 * DT + 1e-6) == []
    for r in more[1:]:
        assert not r.event_mask[1].any() and r.event_mask[0].any() and float(r.flow[0].abs().max()) > 0
    for k, r in enumerate(more[:1]):  # window 2 holds both cameras' events: the loader-equal flow
        assert torch.equal(r.flow, g1[2][0]) and torch.equal(r.event_mask, g1[2][1])
    # a result whose row has been reused raises on access; one that still owns its row does not
    rig = _rig(sd0, 2, slots=2)
    upto = [int(np.searchsorted(c[2], T0 + DT)) + 1 for c in cams]
    first = rig.push([tuple(col[:n] for col in c) for c, n in zip(cams, upto)])[0]
    kept = first.flow.clone()
    till = [int(np.searchsorted(c[2], T0 + 3 * DT)) + 1 for c in cams]
    second, third = rig.push([tuple(col[a:n] for col in c) for c, a, n in zip(cams, upto, till)])
    for access in (lambda: first.flow, lambda: first.event_mask, lambda: first.flow_masked):
        with pytest.raises(_lib.EvflowError, match="reused"):
            access()
    assert torch.equal(kept, g1[0][0]) and torch.equal(second.flow, g1[1][0]) and torch.equal(third.flow, g1[2][0])
    # cameras=1 equals camera 0 of a rig of two whose second camera receives the same events: slots are independent
    one = _feed(_rig(sd0, 1), cams[:1], _few(cams[:1]))
    two = _feed(_rig(sd0, 2), [cams[0], cams[0]], _by_time([cams[0], cams[0]], 1.3 * DT))
    torch.cuda.synchronize()
    assert len(one) == len(two) == NWIN
    for k, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]), k
        assert torch.equal(b[0][0], b[0][1]) and torch.equal(b[1][0], b[1][1]), k
        assert float(a[0].abs().max()) > 0


# ------------------------------------------------------------------ the driver
def test_driver_with_window_dt_in_a_fresh_process_at_two_chunk_sizes(tmp_path):
    """infer_flow.py --window-dt with one file per camera, --out at --chunk 53 and --chunk 700: byte-identical .npy files."""
    import infer_flow
    from event_flow_amd.configs.parser import YAMLParser
    from event_flow_amd.models.model import MODELS

    cams = [_camera(0), _camera(1)]
    names = _files(tmp_path / "data", cams)
    tcfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    tcfg["loader"].update(resolution=[H, W], gpu=0)
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path / "data"), mode="time", window=DT)
    ecfg["loader"].update(batch_size=2, resolution=[H, W])
    ecfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))
    args = type("Args", (), {"train_config": str(tmp_path / "train.yml")})()
    config = infer_flow.merged_config(args, YAMLParser(str(tmp_path / "eval.yml")))
    torch.manual_seed(4)
    model = MODELS[config["model"]["name"]](config["model"].copy()).to(DEV)
    model.eval()
    torch.save(copy.deepcopy(model.state_dict()), tmp_path / "weights.pth")

    outs = {}
    for chunk in (53, 700):
        out = tmp_path / f"out{chunk}"
        cmd = [sys.executable, os.path.join(ROOT, "infer_flow.py"), "--config", str(tmp_path / "eval.yml"), "--train-config",
               str(tmp_path / "train.yml"), "--weights", str(tmp_path / "weights.pth"), "--sequence", names[0], "--sequence", names[1],
               "--window-dt", str(DT), "--max-events", str(NPAD), "--chunk", str(chunk), "--out", str(out)]
        ran = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
        line = json.loads(ran.stdout.strip().splitlines()[-1])
        print(chunk, line)
        assert (line["windows"], line["cameras"], line["chunk"], line["events"]) == (NWIN, 2, chunk, [len(c[0]) for c in cams])
        assert line["stream"]["replayed"] == NWIN - 2 and line["stream"]["graph_a"] >= 1 and line["stream"]["graph_b"] >= 1
        files = sorted(os.listdir(out))
        assert files == ["flow_%06d.npy" % k for k in range(NWIN)]
        outs[chunk] = [open(out / f, "rb").read() for f in files]
        flows = [np.load(out / f) for f in files]
        assert all(f.shape == (2, 2, H, W) and np.abs(f).max() > 0 for f in flows)
    assert outs[53] == outs[700]
