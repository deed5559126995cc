"""Device-resident evaluation loader on the MI355X (event_flow_amd/dataloader/resident_eval.py, csrc/evf_resident_eval.hip): the
four kernels through the C ABI against the loader's host functions, the loader's batches against H5Loader's on the same files,
config and RNG state in the modes time / frames / gtflow_dt1 / gtflow_dt4, and the evaluation driver with and without
--resident."""

import os
import types

import numpy as np
import pytest
import torch
import yaml

from test_gpu_resident import _seeded, det_on  # noqa: F401  (det_on: fixture)
from test_host_loader import _cfg
from test_host_resident import FLIPS
from test_host_resident_eval import CASES, RES, gap_file, three_timed_files

from event_flow_amd import _lib
from event_flow_amd.dataloader.base import BaseDataLoader
from event_flow_amd.dataloader.encodings import binary_search_array
from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_ALIVE = []  # device copies made by _dev: an argument built inside a call must outlive the launch that reads its address


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _dev(a):
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return _ALIVE[-1]


def _host(res, flags):
    """The loader's host functions (event_formatting, augment_*, create_list_encoding) for one slot with these flip flags."""
    ld = BaseDataLoader.__new__(BaseDataLoader)
    ld.res = tuple(res)
    ld.batch_augmentation = {m: [bool(flags & bit)] for m, bit in zip(FLIPS, (1, 2, 4))}
    return ld


# ------------------------------------------------------------------ evf_ts_search
def test_ts_search_is_binary_search_array():
    """Segments of 1, 37 and 1000 timestamps in one column, the long one with runs of duplicates: every element, midpoints,
    below the first, above the last, and the neighbours of a duplicated value -- the index of the reference's bisection
    (among duplicates NOT searchsorted's)."""
    rng = np.random.Generator(np.random.PCG64(3))
    long = np.sort(rng.random(1000)) * 3.0 + 1e3
    for at, run in ((100, 7), (101 + 7, 2), (500, 33), (990, 10)):
        long[at:at + run] = long[at]
    long = np.sort(long)
    segs = [np.asarray([17.25]), np.sort(rng.random(37)) + 40.0, long]
    col = np.concatenate(segs)
    begin, length, query, want = [], [], [], []
    at = 0
    for s in segs:
        dup = s[len(s) // 2] if len(s) < 1000 else s[500]
        q = np.concatenate([s, (s[:-1] + s[1:]) / 2, [s[0] - 1.0, s[-1] + 1.0, np.nextafter(dup, -np.inf), np.nextafter(dup, np.inf)]])
        begin += [at] * len(q)
        length += [len(s)] * len(q)
        query.append(q)
        want += [binary_search_array(s, v) for v in q]
        at += len(s)
    query = np.concatenate(query)
    assert binary_search_array(long, long[500]) != np.searchsorted(long, long[500]) == 500  # (the bisection meets another duplicate)
    out = torch.full((len(query),), -7, dtype=torch.int64, device=DEV)
    _lib.call("evf_ts_search", _lib.ptr(_dev(col)), len(col), _lib.ptr(_dev(np.asarray(begin, dtype=np.int64))),
              _lib.ptr(_dev(np.asarray(length, dtype=np.int64))), _lib.ptr(_dev(query)), len(query), _lib.ptr(out))
    assert out.cpu().tolist() == want
    # a segment that leaves the column answers -1; bad arguments are refused before a launch
    bad = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.call("evf_ts_search", _lib.ptr(_dev(col)), len(col), _lib.ptr(_dev(np.asarray([len(col) - 3, -1], dtype=np.int64))),
              _lib.ptr(_dev(np.asarray([4, 2], dtype=np.int64))), _lib.ptr(_dev(query[:2])), 2, _lib.ptr(bad))
    assert bad.cpu().tolist() == [-1, -1]
    assert _lib.raw("evf_ts_search", None, len(col), bad.data_ptr(), bad.data_ptr(), bad.data_ptr(), 2, bad.data_ptr()) != 0
    assert _lib.raw("evf_ts_search", bad.data_ptr(), len(col), bad.data_ptr(), bad.data_ptr(), bad.data_ptr(), 0, bad.data_ptr()) != 0


# ------------------------------------------------------------------ evf_seq_cut_ragged
@pytest.fixture(scope="module")
def arena():
    rng = np.random.Generator(np.random.PCG64(8))
    n, (H, W) = 700, (15, 21)
    cols = (rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), np.sort(rng.random(n)) * 0.3 + 2.0,
            rng.integers(0, 2, n).astype(np.uint8))
    return cols, tuple(_dev(c) for c in cols)


def _cut(arena, first, count, flags, npad, H=15, W=21):
    _cols, dev = arena
    J = len(first)
    ev = torch.full((J, npad, 4), 9.0, dtype=torch.float32, device=DEV)
    dt = torch.full((J,), 9.0, dtype=torch.float64, device=DEV)
    _lib.call("evf_seq_cut_ragged", *(_lib.ptr(c) for c in dev), len(_cols[0]), _lib.ptr(_dev(np.asarray(first, dtype=np.int64))),
              _lib.ptr(_dev(np.asarray(count, dtype=np.int32))), _lib.ptr(_dev(np.asarray(flags, dtype=np.int32))), J, npad, H, W,
              _lib.ptr(ev), _lib.ptr(dt))
    return ev.cpu().numpy(), dt.cpu().numpy()


@pytest.mark.parametrize("npad", [300, 301])
def test_ragged_cut_is_the_host_formatting(arena, npad):
    (xs, ys, ts, ps), _ = arena
    first, count = (5, 40, 333), (0, 11, 300)
    for flags in range(8):
        ev, dt = _cut(arena, first, count, [flags] * 3, npad)
        ld = _host((15, 21), flags)
        for j, (f, c) in enumerate(zip(first, count)):
            x, y, t, p = ld.event_formatting(xs[f:f + c], ys[f:f + c], ts[f:f + c], ps[f:f + c])
            x, y, p = ld.augment_events(x, y, p, 0)
            rows = ld.create_list_encoding(x, y, t, p).T
            assert np.array_equal(ev[j, :c].view(np.uint32), rows.view(np.uint32)), (flags, j)  # bit for bit
            assert not ev[j, c:].any(), (flags, j)
            assert dt[j] == (ts[f + c - 1] - ts[f] if c else 0.0), (flags, j)


def test_ragged_cut_refuses_what_it_cannot_read(arena):
    (xs, ys, ts, ps), dev = arena
    n = len(xs)
    #          leaves the arena   count > Npad   negative first   negative count   the last 20 events: fine
    first, count = (n - 10, 0, -1, 5, n - 20), (11, 41, 12, -3, 20)
    ev, dt = _cut(arena, first, count, [0] * 5, 40)
    assert not ev[:4].any() and not dt[:4].any()
    assert ev[4, :20, 3].all() and not ev[4, 20:].any() and dt[4] == ts[-1] - ts[n - 20]
    one = torch.zeros(64, dtype=torch.int64, device=DEV).data_ptr()
    ok = [_lib.ptr(c) for c in dev] + [n, one, one, one, 1, 4, 15, 21, one, one]
    assert _lib.raw("evf_seq_cut_ragged", *ok) == 0
    for at, bad in ((0, None), (5, None), (12, None), (4, 0), (8, 0), (8, 65536), (9, 0), (10, 0), (11, -1)):
        args = list(ok)
        args[at] = bad
        assert _lib.raw("evf_seq_cut_ragged", *args) != 0, at
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the gathers
@pytest.mark.parametrize("H,W", [(15, 21), (16, 20), (16, 32)])  # no 16-byte path / maps only / maps and frames
def test_gathers_are_the_host_flips(H, W):
    rng = np.random.Generator(np.random.PCG64(H * W))
    M, B = 5, 4
    maps = rng.standard_normal((M, 2, H, W)).astype(np.float32)
    frames = rng.integers(0, 256, (M, H, W)).astype(np.uint8)
    idx, nxt, flags = np.asarray([3, 0, 3, 4], np.int32), np.asarray([4, 1, 4, 0], np.int32), np.arange(4, dtype=np.int32)
    got_m = torch.full((B, 2, H, W), 9.0, dtype=torch.float32, device=DEV)
    got_f = torch.full((B, 2, H, W), 9, dtype=torch.uint8, device=DEV)
    _lib.call("evf_gather_flowmaps", _lib.ptr(_dev(maps)), M, _lib.ptr(_dev(idx)), _lib.ptr(_dev(flags)), B, H, W, _lib.ptr(got_m))
    _lib.call("evf_gather_frames", _lib.ptr(_dev(frames)), M, _lib.ptr(_dev(idx)), _lib.ptr(_dev(nxt)), _lib.ptr(_dev(flags)), B, H, W,
              _lib.ptr(got_f))
    for b in range(B):
        ld = _host((H, W), int(flags[b]))
        assert np.array_equal(got_m[b].cpu().numpy().view(np.uint32), ld.augment_flowmap(maps[idx[b]], 0).view(np.uint32)), b
        want = np.stack([ld.augment_frames(frames[idx[b]], 0), ld.augment_frames(frames[nxt[b]], 0)])
        assert np.array_equal(got_f[b].cpu().numpy(), want), b
    # an index outside the stack gives zeros; bad arguments are refused
    _lib.call("evf_gather_flowmaps", _lib.ptr(_dev(maps)), M, _lib.ptr(_dev(np.asarray([M, -1, 0, 0], np.int32))), _lib.ptr(_dev(flags)),
              B, H, W, _lib.ptr(got_m))
    assert not got_m[:2].any() and got_m[2].any()
    p = got_m.data_ptr()
    assert _lib.raw("evf_gather_flowmaps", None, M, p, p, B, H, W, p) != 0 and _lib.raw("evf_gather_flowmaps", p, 0, p, p, B, H, W, p) != 0
    assert _lib.raw("evf_gather_frames", p, M, p, None, p, B, H, W, p) != 0 and _lib.raw("evf_gather_frames", p, M, p, p, p, B, 0, W, p) != 0


# ------------------------------------------------------------------ the loader
def _run(cls, cfg, seed, passes=2, **kw):
    """(one loader after the other: both draw their flags from numpy's global generator)"""
    ld = _seeded(cls, seed, cfg, 5, **kw)
    out = []
    for _ in range(passes):
        for batch in ld:
            out.append((batch, (ld.new_seq, ld.pass_done, ld.seq_num, ld.samples, float(ld.last_proc_timestamp))))
        out.append((None, (ld.epoch, ld.seq_num, list(ld.batch_idx), list(ld.batch_row))))
    return out, ld


def _equal_runs(want, got, what):
    assert len(got) == len(want)
    for n, ((x, sx), (y, sy)) in enumerate(zip(want, got)):
        assert sx == sy, (what, n, sx, sy)
        assert (x is None) == (y is None)
        if x is not None:
            assert set(x) == set(y), (what, n)
            for k in x:
                assert y[k].is_cuda and x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and torch.equal(x[k], y[k]), (what, n, k)


@pytest.mark.parametrize("mode,window,gap", [c + (False,) for c in CASES] + [("time", 0.25, True)])
def test_every_tensor_equals_h5loaders(tmp_path, det_on, mode, window, gap):  # noqa: F811
    """Three files of 4000 / 3000 / 2500 events (or the file with a gap in place of the second), two slots, all flips, hot
    filter, two passes: torch.equal in every tensor of every batch, gtflow / frames included, same flags, counters and
    last_proc_timestamp."""
    three_timed_files(tmp_path)
    if gap:
        os.remove(tmp_path / "s1.npz")
        gap_file(tmp_path / "s1.npz")
    cfg = _cfg(tmp_path, mode, window, 2, RES, FLIPS, hot=True)
    extra = {"time": set(), "frames": {"frames"}}.get(mode, {"gtflow"})
    ragged = padded = restarts = 0
    for seed in (0, 3):
        (want, _), (got, ld) = _run(H5Loader, cfg, seed, prefetch=0), _run(ResidentEvalLoader, cfg, seed)
        _equal_runs(want, got, (mode, window, seed))
        per_event = 13 * ld.total_events + 4 * (2 * RES[0] * RES[1] + 2)
        per_item = {"time": 0, "frames": RES[0] * RES[1]}.get(mode, 8 * RES[0] * RES[1])
        assert ld.resident_bytes == per_event + 12 * per_item
        for x, s in want:
            if x is None:
                continue
            assert set(x) == {"event_cnt", "event_voxel", "event_mask", "event_list", "event_list_pol_mask", "dt_gt", "dt_input"} | extra
            restarts += s[0]
            n = (x["event_list"][:, :, 3] != 0).sum(1)  # events per slot
            ragged += int(n[0] != n[1])
            padded += int(n.min() == 0 and n.max() > 0)
    assert restarts >= 3
    if mode == "time":
        assert ragged >= 3
    if gap:
        assert padded >= 1


def test_a_batch_of_empty_windows(tmp_path, det_on):  # noqa: F811
    """One slot on the file with a gap: the windows with five and with no events are batches with empty lists ([1, 0, 4] and
    [1, 0, 2]), and still hot-pixel observations."""
    gap_file(tmp_path / "gap.npz")
    cfg = _cfg(tmp_path, "time", 0.25, 1, RES, FLIPS, hot=True)
    (want, _), (got, _) = _run(H5Loader, cfg, 1, passes=1, prefetch=0), _run(ResidentEvalLoader, cfg, 1, passes=1)
    _equal_runs(want, got, "gap")
    shapes = [tuple(y["event_list"].shape) for y, _ in got if y is not None]
    assert shapes.count((1, 0, 4)) == 2 and tuple(got[2][0]["event_list_pol_mask"].shape) == (1, 0, 2)


# ------------------------------------------------------------------ the driver
def test_evaluation_with_and_without_resident(tmp_path, det_on):  # noqa: F811
    """eval_flow.test on two moving-dots sequences with ground-truth maps, data.mode gtflow_dt1, LIFFireNet, AEE + FWL + RSAT,
    deterministic mode: the same results with H5Loader and with --resident.  A key that does not reproduce between two H5Loader
    runs is compared at four times that observed difference."""
    import eval_flow
    from event_flow_amd import synthetic
    from event_flow_amd.configs.parser import YAMLParser

    H, W = 32, 40
    (tmp_path / "data").mkdir()
    for i in range(2):
        xs, ys, ts, ps, (u, v) = synthetic.moving_dots_events(5000, H, W, 40 + i, max_disp=20.0)
        ts = ts * 0.6 + 5.0
        stamps = 5.0 + 0.1 * np.arange(7)
        gt = np.zeros((2, H, W), np.float32)
        gt[0], gt[1] = u / 6, v / 6
        write_npz_sequence(str(tmp_path / "data" / f"seq{i}.npz"), xs.astype(np.int16), ys.astype(np.int16), ts, (ps > 0).astype(np.int8),
                           flow_dt1=[(f"{k:06d}", stamps[k], gt * (1 + 0.1 * k)) for k in range(7)])
    root = os.path.dirname(os.path.abspath(eval_flow.__file__))
    tcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    tcfg["loader"].update(resolution=[H, W])
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    ecfg = yaml.safe_load(open(os.path.join(root, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path / "data"), mode="gtflow_dt1", window=1, window_eval=200)
    ecfg["loader"].update(resolution=[H, W])
    ecfg["metrics"]["name"] = ["AEE", "FWL", "RSAT"]
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))

    def run(resident):
        torch.manual_seed(4)
        np.random.seed(4)
        args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", synthetic=False, sequences=4,
                                     resident=resident, store="")
        return eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")))

    a, a2, b = run(False), run(False), run(True)
    assert set(a) == set(b) >= {"AEE", "AEE_percent_outliers", "FWL", "RSAT", "iwe_variance"}
    assert np.isfinite(a["AEE"]) and a["AEE"] > 0
    for k in a:
        print(k, a[k], a2[k], b[k])
        if isinstance(a[k], str):
            assert a[k] == b[k]
        else:
            assert abs(a[k] - b[k]) <= 4 * abs(a[k] - a2[k]), (k, a[k], a2[k], b[k])
