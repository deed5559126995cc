"""Device-resident sequence loader on the MI355X (event_flow_amd/dataloader/resident.py, csrc/evf_resident.hip): its batches
against the reference-made fixture G13 and against H5Loader on the same files, flags and RNG state; the hot-pixel selection
past max_px; whole windows from one launch; the training driver with and without --resident."""

import copy
import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

from test_host_loader import _cfg, _g13_files
from test_host_resident import FLIPS, driver_groups, three_files

from event_flow_amd import _lib
from event_flow_amd.dataloader import encodings
from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence
from event_flow_amd.dataloader.resident import ResidentLoader

pytestmark = pytest.mark.gpu
KEYS = {"event_cnt", "event_voxel", "event_mask", "event_list", "event_list_pol_mask", "dt_gt", "dt_input"}


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def _seeded(cls, seed, *a, **kw):
    np.random.seed(seed)
    random.seed(seed)
    ld = cls(*a, **kw)
    ld.shuffle()
    return ld


def _same_batch(a, b, what):
    assert set(a) == set(b) == KEYS, what
    for k in KEYS:
        assert a[k].is_cuda and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("N", [11, 257])  # the smallest window the loader admits / past one block of 256 threads
def test_seq_cut_is_the_host_formatting(N):
    """evf_seq_cut through the C ABI on an arena of 700 events at 15 x 21, B = 2, P = 3 (job j = b * P + p), every flip flag on
    every job: rows bit for bit the loader's host functions on the host slice, dt[p, b] the slice's span; the last readable
    window; a window one event past the arena and a negative first come back as zero rows with dt = 0."""
    from event_flow_amd.dataloader.base import BaseDataLoader

    rng = np.random.Generator(np.random.PCG64(8))
    n, (H, W), B, P = 700, (15, 21), 2, 3
    xs, ys, ts, ps = cols = (rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16),
                             np.sort(rng.random(n)) * 0.3 + 2.0, rng.integers(0, 2, n).astype(np.uint8))
    dev = [torch.from_numpy(c).cuda() for c in cols]
    first = [0, 40, n - N, n - N + 1, -1, 333]
    first_dev = torch.tensor(first, dtype=torch.int64).cuda()
    host = BaseDataLoader.__new__(BaseDataLoader)
    host.res = (H, W)
    for sweep in range(8):
        flags = [(sweep + j) & 7 for j in range(B * P)]
        flags_dev = torch.tensor(flags, dtype=torch.int32).cuda()
        ev = torch.full((B, P, N, 4), 9.0, dtype=torch.float32, device="cuda")
        dt = torch.full((P, B), 9.0, dtype=torch.float64, device="cuda")
        _lib.call("evf_seq_cut", *(_lib.ptr(c) for c in dev), n, _lib.ptr(first_dev), _lib.ptr(flags_dev), B, P, N, H, W,
                  _lib.ptr(ev), _lib.ptr(dt))
        ev, dt = ev.cpu().numpy(), dt.cpu().numpy()
        for j, (f, fl) in enumerate(zip(first, flags)):
            b, p = divmod(j, P)
            if f < 0 or f > n - N:
                assert not ev[b, p].any() and dt[p, b] == 0.0, (sweep, j)
                continue
            host.batch_augmentation = {m: [bool(fl & bit)] for m, bit in zip(FLIPS, (1, 2, 4))}
            x, y, t, pol = host.event_formatting(xs[f:f + N], ys[f:f + N], ts[f:f + N], ps[f:f + N])
            x, y, pol = host.augment_events(x, y, pol, 0)
            rows = host.create_list_encoding(x, y, t, pol).T
            assert np.array_equal(ev[b, p].view(np.uint32), rows.view(np.uint32)), (sweep, j)  # bit for bit
            assert dt[p, b] == ts[f + N - 1] - ts[f], (sweep, j)
    # bad arguments are refused before a launch; an empty arena is not one (every job is padding)
    out_ev, out_dt = torch.zeros((1, 1, 4, 4), dtype=torch.float32, device="cuda"), torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    ok = [_lib.ptr(c) for c in dev] + [n, _lib.ptr(first_dev), _lib.ptr(flags_dev), 1, 1, 4, H, W, _lib.ptr(out_ev), _lib.ptr(out_dt)]
    assert _lib.raw("evf_seq_cut", *ok) == 0
    assert _lib.raw("evf_seq_cut", *ok[:4], 0, *ok[5:]) == 0
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (4, -1), (5, None), (6, None), (7, 0), (7, 65536), (8, 0), (9, 0),
                    (10, 0), (11, 0), (12, None), (13, None)):
        args = list(ok)
        args[at] = bad
        assert _lib.raw("evf_seq_cut", *args) != 0, at
    torch.cuda.synchronize()


def test_batches_match_the_reference_collate(tmp_path):
    """Fixture G13 (the reference's loader code: flips and hot-pixel filter on) at the bars of tests/test_gpu_loader.py."""
    g, (H, W, win, nwin, nb) = _g13_files(tmp_path)
    ld = ResidentLoader(_cfg(tmp_path, "events", win, 2, (H, W), FLIPS, hot=True), nb)
    ld.batch_augmentation = {k: [bool(v) for v in g["aug_" + k]] for k in FLIPS}
    assert ld.resident_bytes == 13 * ld.total_events and ld.total_events == 2 * (win * nwin + 37)
    seen = 0
    for w, batch in enumerate(ld):
        if w < nwin:
            assert not ld.new_seq and not ld.pass_done
            assert set(batch) == KEYS
            for k, v in batch.items():
                ref = g[f"w{w}_{k}"]
                assert v.is_cuda and tuple(v.shape) == ref.shape and str(v.dtype).split(".")[-1] == str(ref.dtype), k
                if k == "event_voxel":  # sums of fp32 temporal weights: equal up to the order of the atomic adds
                    np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=0, atol=2e-6, err_msg=f"{w} {k}")
                    assert np.array_equal(v.cpu().numpy() == 0, ref == 0)
                else:  # integer-valued images and fp32 copies: bit for bit
                    assert np.array_equal(v.cpu().numpy(), ref), (w, k)
            assert ld.last_proc_timestamp == float(g["seq1_ts"][(w + 1) * win - 1] - g["seq1_ts"][0])
        else:  # both slots ran out of events: first windows of the next files, fresh augmentation flags
            assert ld.new_seq and ld.pass_done and w == nwin
            assert tuple(batch["event_list"].shape) == (2, win, 4)
        seen += 1
    assert seen == nwin + 1 and ld.epoch == 1 and ld.seq_num == 0 and ld.samples == 2 * (nwin + 1) and not ld.new_seq


def test_every_tensor_equals_h5loaders(tmp_path, det_on):
    """Three files of 1537 / 1000 / 700 events, windows of 300, two slots, all flips, hot filter, two passes over the files:
    torch.equal in every tensor of every batch (the exact-sum voxel binning does not depend on the order), same flags and
    counters."""
    three_files(tmp_path)
    cfg = _cfg(tmp_path, "events", 300, 2, (16, 20), FLIPS, hot=True)

    def run(cls, seed, **kw):  # (one loader after the other: both draw their flags from numpy's global generator)
        ld = _seeded(cls, seed, cfg, 5, **kw)
        out = []
        for _ in range(2):
            for batch in ld:
                out.append((batch, (ld.new_seq, ld.pass_done, ld.seq_num, ld.samples, float(ld.last_proc_timestamp))))
            out.append((None, (ld.epoch, ld.seq_num, list(ld.batch_idx), list(ld.batch_row))))
        return out

    for seed in (0, 3):
        want, got = run(H5Loader, seed, prefetch=0), run(ResidentLoader, seed)
        assert len(got) == len(want) >= 10
        for n, ((x, sx), (y, sy)) in enumerate(zip(want, got)):
            assert sx == sy, (seed, n)
            assert (x is None) == (y is None)
            if x is not None:
                _same_batch(y, x, (seed, n))
        assert sum(s[0] for x, s in want if x is not None) >= 3  # (batches with a restarted slot)


def _planted_file(path, seed, planted, H=16, W=20, windows=6, win=300):
    """`windows` windows of `win` events (+ a short tail): pixel q of `planted` = {q: first window it fires in} has one event
    in every window from then on; the rest of a window falls on 12 other pixels, new ones in every window."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xs, ys = [], []
    free = rng.permutation(np.setdiff1d(np.arange(H * W), list(planted)))
    for w in range(windows + 1):
        q = [p for p, since in planted.items() if w >= since] if w < windows else []
        n = (win if w < windows else 40) - len(q)
        q = np.concatenate([np.asarray(q, dtype=np.int64), rng.choice(free[12 * w:12 * w + 12], n)])
        q = rng.permutation(q)
        xs.append(q % W)
        ys.append(q // W)
    n = sum(len(x) for x in xs)
    write_npz_sequence(str(path), np.concatenate(xs), np.concatenate(ys), np.sort(rng.random(n)) + 3.0, rng.integers(0, 2, n))


PLANTED = {  # (H, W): (first file {pixel: first window}, second file, cleared in window six of the first, cleared in the second)
    (16, 20): ({25: 0, 290: 0, 47: 1, 131: 1, 208: 1, 77: 2}, {12: 0, 13: 0, 300: 0, 301: 0, 150: 0, 5: 0}, {25, 290, 47}, {5, 12, 13}),
    # 2080 pixels: a thread of the index-ordered pass owns three consecutive pixels (the last threads none); ties inside one
    # thread's pixels (1030, 1031) and in the next thread's (1033)
    (40, 52): ({30: 0, 2079: 0, 1030: 1, 1031: 1, 1033: 1, 500: 2}, {2078: 0, 2077: 0, 3: 0, 4: 0, 5: 0, 1500: 0}, {30, 2079, 1030}, {3, 4, 5}),
}


@pytest.mark.parametrize("res", sorted(PLANTED))
def test_hot_filter_beyond_max_px(tmp_path, det_on, res):
    """max_px = 3 with six planted pixels: two fire in all six windows, three from the second window on (rate 4/5 = max_rate in
    window five: not above it; 5/6 in window six: tied at the cut, the lowest flat index is taken), one from the third on.
    Every tensor equals H5Loader's over both files (the statistics reset at the restart) and the cleared pixels are the
    expected ones."""
    (H, W), (A, Bp, six, second) = res, PLANTED[res]
    always = {q for q, since in A.items() if since == 0}
    _planted_file(tmp_path / "s0.npz", 1, A, H, W)
    _planted_file(tmp_path / "s1.npz", 2, Bp, H, W)  # second file: six pixels at rate 1 from its first window on
    cfg = _cfg(tmp_path, "events", 300, 1, (H, W), hot=True)
    cfg["hot_filter"].update(max_px=3, min_obvs=2, max_rate=0.8)
    ref, ld = H5Loader(cfg, 5, prefetch=0), ResidentLoader(cfg, 5)  # (no augmentation: neither draws random numbers)
    cleared = []
    for w, (x, y) in enumerate(zip(ref, ld)):
        _same_batch(y, x, w)
        assert ld.new_seq == ref.new_seq == (w in (6, 12))
        ev = y["event_list"][0].cpu().numpy()
        hit = np.zeros(H * W, bool)
        hit[(ev[:, 1] * W + ev[:, 2]).astype(int)] = True
        cleared.append(set(np.flatnonzero(hit & (y["event_mask"][0, 0].cpu().numpy().reshape(-1) == 0))))
    assert w == 12
    assert cleared[:6] == [set(), set(), always, always, always, six]
    assert cleared[6:12] == [set(), set()] + [second] * 4 and cleared[12] == set()


def test_next_window_is_the_training_loops_group_of_batches(tmp_path, det_on):
    """next_window(3) against the per-pass iterator of a second loader with the same seed, grouped like train_flow.py's loop:
    same tensors (the dropped batches' hot-pixel observations included), `reset` where the loop reset, and the loss inputs are
    in-place slices of window buffers."""
    three_files(tmp_path, lengths=(2750, 1900, 1300))
    cfg = _cfg(tmp_path, "events", 300, 2, (16, 20), FLIPS, hot=True)
    per_pass = _seeded(ResidentLoader, 5, cfg, 5)
    batches, restarts = [], []
    for _ in range(3):
        for batch in per_pass:
            batches.append(batch)
            restarts.append(per_pass.new_seq)
    groups = driver_groups(restarts, 3)
    assert len(groups) >= 3 and any(r for _, r in groups) and any(not r for _, r in groups)
    assert any(a[-1] + 1 != b[0] for (a, _), (b, _) in zip(groups, groups[1:]))  # (batches were dropped in between)
    ld = _seeded(ResidentLoader, 5, cfg, 5)
    for idx, reset in groups:
        passes, got_reset = ld.next_window(3)
        assert got_reset == reset and len(passes) == 3
        for p, i in enumerate(idx):
            _same_batch(passes[p], batches[i], (idx, p))
        for k in ("event_list", "event_list_pol_mask", "event_mask"):
            base = encodings.window_base([d[k] for d in passes])
            assert base is not None and base.shape[:2] == (2, 3), k
    assert ld.samples == 2 * (groups[-1][0][-1] + 1)


def test_training_with_and_without_resident(tmp_path, det_on):
    """train_flow.train on the same files and seeds, H5Loader against --resident, deterministic mode: LIFFireNet, cnt encoding,
    2 x 32 x 40, passes of 400 events, window_loss 1200, FlatAdam -- equal per-epoch losses and equal parameters."""
    import train_flow
    from event_flow_amd.configs.parser import YAMLParser

    (tmp_path / "data").mkdir()
    three_files(tmp_path / "data", H=32, W=40, lengths=(4100, 3300, 2900))
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(train_flow.__file__)), "configs", "train_SNN.yml")))
    cfg["data"].update(path=str(tmp_path / "data"), window=400, window_loss=1200)
    cfg["loader"].update(batch_size=2, n_epochs=2, resolution=[32, 40], augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
    cfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    cfg["vis"]["verbose"] = False
    yaml.safe_dump(cfg, open(tmp_path / "train.yml", "w"))
    runs = []
    for resident in (False, True):
        out = str(tmp_path / f"m{int(resident)}.pth")
        args = types.SimpleNamespace(synthetic=False, prev="", out=out, epochs=2, fused_optimizer=True, resident=resident)
        np.random.seed(9)
        random.seed(9)
        history = train_flow.train(args, YAMLParser(str(tmp_path / "train.yml")))
        runs.append((copy.deepcopy(history), torch.load(out, map_location="cpu")))
    (h0, sd0), (h1, sd1) = runs
    assert len(h0) == 2 and all(np.isfinite(v) and v > 0 for v in h0), h0
    assert h0 == h1
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
