"""Streaming inference on the MI355X (event_flow_amd/stream.py, csrc/evf_stream.hip, infer_flow.py): evf_ring_append against a
numpy ring across the wrap, evf_ring_cut against evf_seq_cut on the linear arena of the same events bit for bit, their guards
and a captured replay; `FlowStream` fed one sequence file in several chunkings against the eager evaluation loop on
`ResidentLoader` (B = 1, `events` mode), window by window with torch.equal; replay, reset, the result ring and the refusals; the
driver in a fresh process."""

import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from test_gpu_eval_graphed import NETS, _initial
from test_gpu_deterministic import _model_cfg
from test_host_eval_steps import H, N, W
from test_host_loader import _cfg
from test_host_resident import three_files

from event_flow_amd import _lib
from event_flow_amd.dataloader.h5 import open_sequence
from event_flow_amd.dataloader.resident import ResidentLoader
from event_flow_amd.dataloader.resident_base import read_columns
from event_flow_amd.stream import FlowStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 2 * N + 37
EVENTS = 9100  # 22 windows of N = 400 events and 300 left over
CANARY = 8     # elements in front of and behind every column


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def _events(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), np.sort(rng.random(n)) * 0.7 + 3.0,
            rng.integers(0, 2, n).astype(np.uint8))


def _chunk_bytes(head, xs, ys, ts, ps):
    """The staged buffer of one append: the int64 head word, then ts | xs | ys | ps."""
    return np.concatenate([np.array([head], dtype=np.int64).view(np.uint8), ts.view(np.uint8), xs.view(np.uint8), ys.view(np.uint8), ps])


def _guarded(dtype, n, fill):
    """A column of n elements with CANARY elements in front of and behind it -> (whole tensor, pointer of the column)."""
    t = torch.full((n + 2 * CANARY,), fill, dtype=torch.int16 if dtype == torch.uint16 else dtype, device=DEV)  # (uint16 bits)
    return t, t.data_ptr() + CANARY * t.element_size()


def _ring_of(cols, appended, cap):
    """The ring after `appended` events of `cols` went in, as host arrays: event e at slot e mod cap."""
    out = [np.zeros(cap, dtype=c.dtype) for c in cols]
    ids = np.arange(max(appended - cap, 0), appended)
    for o, c in zip(out, cols):
        o[ids % cap] = c[ids]
    return out


# ------------------------------------------------------------------ evf_ring_append
def test_append_across_the_wrap_equals_a_numpy_ring():
    xs, ys, ts, ps = cols = _events(3 * R, 31)
    fills = (0x7A7A, 0x7A7A, -77.25, 0x7A)
    dev = [_guarded(dt, R, f) for dt, f in zip((torch.uint16, torch.uint16, torch.float64, torch.uint8), fills)]
    ref = [np.full(R, f, dtype=c.dtype) for c, f in zip(cols, fills)]
    stage = torch.zeros(8 + 13 * R + 16, dtype=torch.uint8, device=DEV)
    head = 0
    for n in (1, 7, N, R, 1, 7, N, R):
        sl = slice(head, head + n)
        host = _chunk_bytes(head, xs[sl], ys[sl], ts[sl], ps[sl])
        stage.fill_(0xEE)
        stage[:len(host)].copy_(torch.from_numpy(host))
        at = stage.data_ptr()
        _lib.call("evf_ring_append", at + 8, n, at, dev[0][1], dev[1][1], dev[2][1], dev[3][1], R)
        ids = np.arange(head, head + n)
        for r, c in zip(ref, cols):
            r[ids % R] = c[ids]
        head += n
        for (t, _p), r, f, name in zip(dev, ref, fills, ("xs", "ys", "ts", "ps")):
            got = t.cpu().numpy().view(r.dtype)
            assert np.array_equal(got[CANARY:-CANARY], r), (name, head)
            assert np.all(got[:CANARY] == r.dtype.type(f)) and np.all(got[-CANARY:] == r.dtype.type(f)), ("canary", name, head)
        assert np.all(stage.cpu().numpy()[len(host):] == 0xEE)
    assert head >= 2 * R  # at least two wraps
    # a negative head word writes nothing; no events launch nothing
    before = [t.clone() for t, _p in dev]
    stage[:8].copy_(torch.from_numpy(np.array([-1], dtype=np.int64).view(np.uint8)))
    _lib.call("evf_ring_append", at + 8, 7, at, dev[0][1], dev[1][1], dev[2][1], dev[3][1], R)
    _lib.call("evf_ring_append", at + 8, 0, at, dev[0][1], dev[1][1], dev[2][1], dev[3][1], R)
    assert all(torch.equal(b, t) for b, (t, _p) in zip(before, dev))


# ------------------------------------------------------------------ evf_ring_cut
def _seq_cut(lin, total, first, flags, n_win):
    J = len(first)
    ev = torch.full((1, J, n_win, 4), 9.0, dtype=torch.float32, device=DEV)
    dt = torch.full((J, 1), 9.0, dtype=torch.float64, device=DEV)
    first_dev, flags_dev = torch.tensor(first, dtype=torch.int64, device=DEV), torch.tensor(flags, dtype=torch.int32, device=DEV)
    _lib.call("evf_seq_cut", *(_lib.ptr(c) for c in lin), total, _lib.ptr(first_dev), _lib.ptr(flags_dev), 1, J, n_win, H, W,
              _lib.ptr(ev), _lib.ptr(dt))
    torch.cuda.synchronize()  # (the table tensors live until the launch has read them)
    return ev, dt


def _ring_cut(ring, cap, first, appended, flags, n_win):
    J = len(first)
    words = torch.tensor(list(first) + [appended], dtype=torch.int64, device=DEV)
    ev = torch.full((1, J, n_win, 4), 9.0, dtype=torch.float32, device=DEV)
    dt = torch.full((J, 1), 9.0, dtype=torch.float64, device=DEV)
    flags_dev = torch.tensor(flags, dtype=torch.int32, device=DEV)
    _lib.call("evf_ring_cut", *(_lib.ptr(c) for c in ring), cap, words.data_ptr(), words.data_ptr() + 8 * J, _lib.ptr(flags_dev), 1, J,
              n_win, H, W, _lib.ptr(ev), _lib.ptr(dt))
    torch.cuda.synchronize()  # (the table tensors live until the launch has read them)
    return ev, dt


CUTS = {  # name -> (window, ring capacity, events appended, firsts): the ring holds events [appended - capacity, appended)
    # straddles the wrap (slots 663 .. 836, 0 .. 225) | ends on the ring's last slot | starts on slot 0 after two wraps
    "N": (N, R, 2100, [1500, 2 * R - N, 2 * R]),
    "N=R": (R, R, 2100, [2100 - R]),                   # the whole ring, from the slot behind the head round to the head
    "N=2": (2, R, 2100, [2 * R - 1, 2 * R - 2, 2 * R]),  # slots (836, 0) | (835, 836) | (0, 1)
}


@pytest.mark.parametrize("case", sorted(CUTS))
def test_cut_equals_seq_cut_on_the_linear_arena(case):
    n_win, cap, appended, first = CUTS[case]
    cols = _events(3 * R, 32)
    lin = [torch.from_numpy(c).to(DEV) for c in cols]
    ring = [torch.from_numpy(c).to(DEV) for c in _ring_of(cols, appended, cap)]
    for f in first:
        assert appended - cap <= f and f + n_win <= appended
    for flag in range(8):
        flags = [flag] * len(first)
        ev, dt = _ring_cut(ring, cap, first, appended, flags, n_win)
        want_ev, want_dt = _seq_cut(lin, len(cols[0]), first, flags, n_win)
        assert float(want_ev.abs().max()) > 0 and not torch.any(want_ev[..., 3] == 0)  # live rows, no padding
        assert torch.equal(ev.view(torch.int32), want_ev.view(torch.int32)), (case, flag)  # bit for bit
        assert torch.equal(dt.view(torch.int64), want_dt.view(torch.int64)) and float(dt.min()) > 0, (case, flag)


def test_cut_guard_einval_and_captured_replay():
    cols = _events(3 * R, 33)
    appended = 2100
    lin = [torch.from_numpy(c).to(DEV) for c in cols]
    ring = [torch.from_numpy(c).to(DEV) for c in _ring_of(cols, appended, R)]
    # -- the kernel's own guard: job 0 is partly overwritten / partly unwritten / negative, job 1 is fine
    for bad in (appended - R - 1, appended - N + 1, -1, appended, -(2 ** 40)):
        J, first = 2, [bad, 1500]
        words = torch.tensor(first + [appended], dtype=torch.int64, device=DEV)
        flags = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
        ev, ev_ptr = _guarded(torch.float32, J * N * 4, 9.0)
        dt, dt_ptr = _guarded(torch.float64, J, 9.0)
        assert ev_ptr % 16 == 0
        _lib.call("evf_ring_cut", *(_lib.ptr(c) for c in ring), R, words.data_ptr(), words.data_ptr() + 16, _lib.ptr(flags), 1, J, N, H,
                  W, ev_ptr, dt_ptr)
        want_ev, want_dt = _seq_cut(lin, len(cols[0]), [1500], [5], N)
        rows = ev[CANARY:-CANARY].view(J, N, 4)
        assert not rows[0].any() and float(dt[CANARY]) == 0.0, bad  # padding rows and dt = 0
        assert torch.equal(rows[1].view(torch.int32), want_ev[0, 0].view(torch.int32)) and float(dt[CANARY + 1]) == float(want_dt[0, 0])
        for t in (ev, dt):  # ... and nothing else
            assert bool((t[:CANARY] == 9.0).all()) and bool((t[-CANARY:] == 9.0).all()), bad
    # a window wider than the ring is all padding, whatever the words say
    ev, dt = _ring_cut(ring, R, [appended - R], appended, [0], R + 1)
    assert not ev.any() and float(dt[0, 0]) == 0.0

    # -- every EVF_EINVAL case
    stage = torch.zeros(8 + 13 * R, dtype=torch.uint8, device=DEV)
    at = stage.data_ptr()
    mut = [c.clone() for c in ring]
    ok = [at + 8, 7, at] + [_lib.ptr(c) for c in mut] + [R]
    assert _lib.raw("evf_ring_append", *ok) == 0
    for i, bad in ((0, None), (2, None), (3, None), (4, None), (5, None), (6, None), (1, -1), (1, R + 1), (7, 0), (7, -5), (0, at + 4),
                   (2, at + 4), (5, _lib.ptr(mut[2]) + 4), (3, _lib.ptr(mut[0]) + 1), (4, _lib.ptr(mut[1]) + 1)):
        args = list(ok)
        args[i] = bad
        assert _lib.raw("evf_ring_append", *args) == -22, ("evf_ring_append", i, bad)
    words = torch.tensor([1500, appended], dtype=torch.int64, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    out_ev = torch.zeros((1, 1, N, 4), dtype=torch.float32, device=DEV)
    out_dt = torch.zeros((1, 1), dtype=torch.float64, device=DEV)
    ok = [_lib.ptr(c) for c in ring] + [R, words.data_ptr(), words.data_ptr() + 8, _lib.ptr(flags), 1, 1, N, H, W, _lib.ptr(out_ev),
                                        _lib.ptr(out_dt)]
    assert _lib.raw("evf_ring_cut", *ok) == 0
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (7, None), (13, None), (14, None), (4, 0), (4, -1),
                   (8, 0), (9, 0), (8, 65536), (10, 0), (11, 0), (12, 0), (10, -3), (5, words.data_ptr() + 4), (6, words.data_ptr() + 12),
                   (13, _lib.ptr(out_ev) + 4)):
        args = list(ok)
        args[i] = bad
        assert _lib.raw("evf_ring_cut", *args) == -22, ("evf_ring_cut", i, bad)

    # -- both calls captured in ONE graph, replayed with changed table words (head, the chunk, first, appended)
    n = 37
    table = torch.zeros(2, dtype=torch.int64, device=DEV)  # first | appended
    flags = torch.tensor([6], dtype=torch.int32, device=DEV)

    def launches(cols_dev, ev, dt):
        _lib.call("evf_ring_append", at + 8, n, at, *(_lib.ptr(c) for c in cols_dev), R)
        _lib.call("evf_ring_cut", *(_lib.ptr(c) for c in cols_dev), R, table.data_ptr(), table.data_ptr() + 8, _lib.ptr(flags), 1, 1, N,
                  H, W, _lib.ptr(ev), _lib.ptr(dt))

    def load(head):
        """Stage events [head, head + n) and a window that ends with them."""
        sl = slice(head, head + n)
        host = _chunk_bytes(head, cols[0][sl], cols[1][sl], cols[2][sl], cols[3][sl])
        stage[:len(host)].copy_(torch.from_numpy(host))
        table.copy_(torch.tensor([head + n - N, head + n], dtype=torch.int64))

    start = 2 * R - 20  # the three appended slices: before the ring's end | across it | behind it
    state = [torch.from_numpy(c).to(DEV) for c in _ring_of(cols, start, R)]
    eager, replayed = [c.clone() for c in state], [c.clone() for c in state]
    ev_e, dt_e = torch.zeros((1, 1, N, 4), device=DEV), torch.zeros((1, 1), dtype=torch.float64, device=DEV)
    ev_r, dt_r = torch.zeros_like(ev_e), torch.zeros_like(dt_e)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    load(start)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        launches(replayed, ev_r, dt_r)
    for k in range(3):
        load(start + k * n)
        launches(eager, ev_e, dt_e)
        graph.replay()
        torch.cuda.synchronize()
        want_ev, want_dt = _seq_cut(lin, len(cols[0]), [start + (k + 1) * n - N], [6], N)
        assert torch.equal(ev_r.view(torch.int32), ev_e.view(torch.int32)) and torch.equal(dt_r, dt_e), k
        assert torch.equal(ev_r.view(torch.int32), want_ev.view(torch.int32)) and float(dt_r) == float(want_dt) > 0, k
        for a, b in zip(eager, replayed):
            assert torch.equal(a, b), k
    want = _ring_of(cols, start + 3 * n, R)
    assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(replayed, want))


# ------------------------------------------------------------------ FlowStream against the loader
def _file(path):
    three_files(path, H=H, W=W, lengths=(EVENTS,))
    name = str(path / "s0.npz")
    seq = open_sequence(name)
    xs, ys, _rel, ps, ts = read_columns(seq, name)
    t0 = float(seq.attrs["t0"])
    seq.close()
    return name, (xs, ys, ts, ps), t0


def _model(kind, sd0):
    cls, neuron = NETS[kind]
    model = cls(_model_cfg(neuron)).to(DEV)
    model.load_state_dict(sd0)
    model.eval()
    assert model.compute_path[0] == "fused", model.compute_path
    return model


def _loader_flows(path, model, hot):
    """eval_flow.py's eager loop on ResidentLoader, B = 1, `events` mode -> per window (flow [2,H,W], event mask [H,W])."""
    ld = ResidentLoader(_cfg(path, "events", N, 1, (H, W), (), hot=hot), 2)
    out = []
    with torch.no_grad():
        for inputs in ld:
            if ld.new_seq:
                ld.new_seq = False
                model.reset_states()
            if ld.pass_done:
                break
            x = model(inputs["event_voxel"], inputs["event_cnt"])
            out.append((x["flow"][-1][0].clone(), inputs["event_mask"][0, 0].clone()))
    return out


def _stream_flows(stream, cols, chunks):
    """Push `cols` in pushes of chunks(stream) events -> per window (flow, mask, result) cloned push by push."""
    out, at, total = [], 0, len(cols[0])
    while at < total:
        n = min(chunks(stream), total - at)
        for r in stream.push(*(c[at:at + n] for c in cols)):
            out.append((r.flow.clone(), r.event_mask.clone(), r))
        at += n
    return out


CHUNKINGS = {"N": lambda s: N, "37": lambda s: 37, "2.5N": lambda s: (5 * N) // 2, "largest": lambda s: s.max_push}


def _config(hot):
    return _cfg("unused", "events", N, 1, (H, W), (), hot=hot)


def _against_the_loader(path, kind, hot):
    name, cols, t0 = _file(path)
    sd0 = _initial(kind)
    want = _loader_flows(path, _model(kind, sd0), hot)
    assert len(want) == EVENTS // N and all(float(f.abs().max()) > 0 for f, _m in want)  # nonzero flow in every window
    assert len({float(f.abs().sum()) for f, _m in want}) == len(want)
    for label, chunks in CHUNKINGS.items():
        stream = FlowStream(_model(kind, sd0), _config(hot), window=N, capacity=R, slots=8, t0=t0)
        got = _stream_flows(stream, cols, chunks)
        torch.cuda.synchronize()
        assert len(got) == len(want) and stream.pending == EVENTS % N and stream.appended == EVENTS, label
        assert stream.appended > 3 * R  # the ring wrapped several times
        for k, ((flow, mask, r), (wf, wm)) in enumerate(zip(got, want)):
            assert torch.equal(flow, wf), (label, "flow of window", k)
            assert torch.equal(mask, wm), (label, "event mask of window", k)
            assert (r.index, r.first) == (k, k * N)
            assert (r.t_first, r.t_last) == (cols[2][k * N] - t0, cols[2][k * N + N - 1] - t0)
        assert stream.stats["replayed"] == len(want) - 2 and stream.stats["windows"] == len(want), (label, stream.stats)
        if label == "largest":
            assert stream.stats["pushes"] == 3 and stream.stats["appends"] > 3  # sliced: 8 windows do not fit a ring of 2 N + 37


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("kind", ["lif", "plif"])
def test_stream_equals_the_loader_deterministic(tmp_path, det_on, kind, hot):
    _against_the_loader(tmp_path, kind, hot)


@pytest.mark.parametrize("kind", ["lif", "plif"])
def test_stream_equals_the_loader_default_mode_count_input(tmp_path, kind):
    """The default (float-atomic) mode: the networks read the count encoding, whose sums of +-1 are exact in any order."""
    assert not _lib.deterministic()
    _against_the_loader(tmp_path, kind, True)


# ------------------------------------------------------------------ replay, reset, refusals
def test_replay_reset_result_ring_and_refusals(tmp_path, det_on):
    name, cols, t0 = _file(tmp_path)
    sd0 = _initial("lif")

    def run(replay, twice=False, slots=8):
        stream = FlowStream(_model("lif", sd0), _config(True), window=N, capacity=R, slots=slots, t0=t0, replay=replay)
        got = _stream_flows(stream, cols, CHUNKINGS["2.5N"])
        if twice:
            assert stream.pending == EVENTS % N
            stream.reset()
            assert (stream.pending, stream.appended, stream.windows) == (0, 0, 0)
            got += _stream_flows(stream, cols, CHUNKINGS["37"])
        torch.cuda.synchronize()
        return stream, got

    s1, g1 = run(True)
    s0, g0 = run(False)
    nw = EVENTS // N
    assert len(g1) == len(g0) == nw
    for k, (a, b) in enumerate(zip(g1, g0)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
    assert s0.stats["eager"] == nw and s0.stats["replayed"] == 0
    assert s1.stats["eager"] == 2 and s1.stats["replayed"] >= nw - 2 and s1.stats["graph_a"] >= 1 and s1.stats["graph_b"] >= 1
    assert s1.stats["graph_a"] + s1.stats["graph_b"] == s1.stats["replayed"] and s1.stats["replayed_reset"] == 0
    # flow_masked is eval_flow.py's flow_vis
    last = g1[-1][2]
    assert s1.model.mask and torch.equal(last.flow_masked, last.flow * last.event_mask)
    assert last.ready.query()
    # reset(): the same file twice gives the first run's flows both times (the second time under the replayed zero-fill)
    s2, g2 = run(True, twice=True)
    assert len(g2) == 2 * nw and s2.stats["replayed_reset"] == 1
    for k in range(nw):
        for half in (g2[k], g2[nw + k]):
            assert torch.equal(half[0], g1[k][0]) and torch.equal(half[1], g1[k][1]), k
        assert g2[nw + k][2].index == k
    # a result whose row has been reused raises on access; one that still owns its row does not
    stream = FlowStream(_model("lif", sd0), _config(True), window=N, capacity=R, slots=2, t0=t0)
    first = stream.push(*(c[:N] for c in cols))[0]
    kept = first.flow.clone()
    second, third = stream.push(*(c[N:3 * N] for c in cols))
    for access in (lambda: first.flow, lambda: first.event_mask, lambda: first.flow_masked):
        with pytest.raises(_lib.EvflowError, match="reused"):
            access()
    assert torch.equal(kept, g1[0][0]) and torch.equal(second.flow, g1[1][0]) and torch.equal(third.flow, g1[2][0])
    # a push that is too long is refused before any device work; so is every bad column
    stream = FlowStream(_model("lif", sd0), _config(True), window=N, capacity=R, slots=2, t0=t0)
    stream.push(*(c[:150] for c in cols))
    state = (stream.appended, stream.pending, stream.windows, dict(stream.stats), stream.ring.copies)
    assert stream.max_push == 2 * N - 150
    bad = {"too long": [c[150:150 + 2 * N - 149] for c in cols], "x = W": [c[150:160].copy() for c in cols],
           "p = 2": [c[150:160].copy() for c in cols], "NaN": [c[150:160].copy() for c in cols],
           "lengths": [cols[0][150:160], cols[1][150:161], cols[2][150:160], cols[3][150:160]]}
    bad["x = W"][0][3] = W
    bad["p = 2"][3][9] = 2
    bad["NaN"][2][0] = np.nan
    for what, push in bad.items():
        with pytest.raises(_lib.EvflowError):
            stream.push(*push)
        assert state == (stream.appended, stream.pending, stream.windows, dict(stream.stats), stream.ring.copies), what
    assert len(stream.push(*(c[150:150 + stream.max_push] for c in cols))) == 2  # the largest push is accepted
    # a general-path network is refused with the eager alternative named
    from event_flow_amd.models.model import FireNet

    os.environ["EVF_PATH_NOTICE"] = "0"
    try:
        ann = FireNet({**_model_cfg({}), "activations": ["relu", None]}).to(DEV)
        with pytest.raises(_lib.EvflowError, match="general path.*encode_event_list"):
            FlowStream(ann, _config(False), window=N)
    finally:
        os.environ.pop("EVF_PATH_NOTICE", None)


# ------------------------------------------------------------------ the driver
def test_driver_in_a_fresh_process_at_two_chunk_sizes(tmp_path):
    """infer_flow.py --out at --chunk 37 and --chunk 1000: byte-identical .npy files, equal to the loader path's flows."""
    import infer_flow
    from event_flow_amd.configs.parser import YAMLParser
    from event_flow_amd.models.model import MODELS

    (tmp_path / "data").mkdir()
    name, cols, t0 = _file(tmp_path / "data")
    tcfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    tcfg["loader"].update(resolution=[H, W], gpu=0)
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path / "data"), mode="events", window=N)
    ecfg["loader"].update(batch_size=1, resolution=[H, W])
    ecfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))
    args = type("Args", (), {"train_config": str(tmp_path / "train.yml")})()
    config = infer_flow.merged_config(args, YAMLParser(str(tmp_path / "eval.yml")))
    torch.manual_seed(4)
    model = MODELS[config["model"]["name"]](config["model"].copy()).to(DEV)
    model.eval()
    torch.save(copy.deepcopy(model.state_dict()), tmp_path / "weights.pth")
    want = _loader_flows(tmp_path / "data", model, True)
    assert len(want) == EVENTS // N and all(float(f.abs().max()) > 0 for f, _m in want)

    outs = {}
    for chunk in (37, 1000):
        out = tmp_path / f"out{chunk}"
        cmd = [sys.executable, os.path.join(ROOT, "infer_flow.py"), "--config", str(tmp_path / "eval.yml"), "--train-config",
               str(tmp_path / "train.yml"), "--weights", str(tmp_path / "weights.pth"), "--sequence", name, "--chunk", str(chunk),
               "--out", str(out)]
        ran = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
        line = json.loads(ran.stdout.strip().splitlines()[-1])
        print(chunk, line)
        assert (line["windows"], line["pending"], line["chunk"], line["events"]) == (EVENTS // N, EVENTS % N, chunk, EVENTS)
        assert line["stream"]["replayed"] == EVENTS // N - 2 and line["stream"]["graph_a"] >= 1 and line["stream"]["graph_b"] >= 1
        assert line["ms_per_window"] > 0
        files = sorted(os.listdir(out))
        assert files == ["flow_%06d.npy" % k for k in range(EVENTS // N)]
        outs[chunk] = [open(out / f, "rb").read() for f in files]
        for k, f in enumerate(files):
            assert np.array_equal(np.load(out / f), want[k][0].cpu().numpy()), (chunk, k)
    assert outs[37] == outs[1000]
