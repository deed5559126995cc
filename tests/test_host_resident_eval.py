"""Host side of the device-resident evaluation loader (event_flow_amd/dataloader/resident_eval.py) without a GPU: the plan over
index tables against what H5Loader's own host code (dataloader/h5.py:240-326) does on the same files, config and RNG state in
the modes time / frames / gtflow_dt1 / gtflow_dt4, the windows that come out empty, and the refusals."""

import random

import numpy as np
import pytest

from test_host_loader import _cfg, _timed_sequence
from test_host_resident import FLIPS, _state

from event_flow_amd import _lib
from event_flow_amd.dataloader.encodings import binary_search_array
from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader, ResidentEvalPlan

B, RES = 2, (16, 20)
LENGTHS = (4000, 3000, 2500)
CASES = [("time", 0.25), ("frames", 1), ("frames", 2), ("frames", 0.5), ("gtflow_dt1", 1), ("gtflow_dt4", 0.25)]
PASSES = 2


def three_timed_files(path, lengths=LENGTHS):
    for k, n in enumerate(lengths):
        _timed_sequence(path / f"s{k}.npz", n=n, seed=30 + k, maps=1, frames=1)


def gap_file(path):
    """A `time`-mode sequence (t0 = 50, windows of 0.25 s): 600 events in [0, 0.5), FIVE in [0.5, 0.75), none in [0.75, 1.0),
    500 in [1.0, 1.6] -> the third window has between 1 and 10 events, the fourth none.  -> its timestamps."""
    rng = np.random.Generator(np.random.PCG64(77))
    ts = np.concatenate([[50.0], 50.0 + np.sort(rng.random(599)) * 0.49 + 0.005, 50.0 + 0.55 + 0.03 * np.arange(5),
                         50.0 + 1.01 + np.sort(rng.random(500)) * 0.59])
    n = len(ts)
    write_npz_sequence(str(path), rng.integers(0, RES[1], n), rng.integers(0, RES[0], n), ts, rng.integers(0, 2, n))
    return ts


class _Recording(H5Loader):
    """H5Loader that remembers, per sample, the file it came from, the cursor it was cut at, whether the slot moved on to
    another file on the way, and the event slice `get_events` was asked for."""

    def _open(self, batch, path):
        d = self.__dict__
        d.setdefault("paths", {})[batch] = path
        d["opens"] = d.get("opens", 0) + 1
        super()._open(batch, path)

    def get_events(self, file, idx0, idx1):
        self.__dict__["cut"] = (idx0, idx1)
        return super().get_events(file, idx0, idx1)

    def __getitem__(self, index):
        b = index % self.batch_size
        opens, row = self.opens, self.batch_row[b]
        s = super().__getitem__(index)
        restarted = self.opens != opens
        s["_rec"] = (self.paths[b], 0 if restarted else row, restarted, self.cut)
        return s


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def h5_trajectory(ld, passes, events):
    """Per batch of `passes` passes over the files: (jobs, restarted, state, last_proc_timestamp); jobs = (path, first, count,
    flags, restarted, indices, dt_gt) per slot -- `_host_batches` with the bookkeeping of `_deliver` (whose collate step
    needs the GPU).  first / count: the slice `get_events` took, clipped to the file, and the width of the sample's rows."""
    out = []
    w = ld.window
    for _ in range(passes):
        for samples, flags in ld._host_batches():
            ld.new_seq, ld.pass_done = flags
            ld.samples += ld.batch_size
            jobs = []
            for b, s in enumerate(samples):
                path, row, restarted, (idx0, _idx1) = s["_rec"]
                indices = None
                if ld.mode == "frames":
                    indices = (int(np.floor(row)), int(np.ceil(row + w)))
                    assert s["frames"].shape == (2,) + RES and s["frames"].dtype == np.uint8
                elif ld.mode != "time":
                    indices = int(np.ceil(row + w))
                    assert s["gtflow"].shape == (2,) + RES
                fl = sum(bit for bit, m in zip((1, 2, 4), FLIPS) if ld.batch_augmentation[m][b])
                jobs.append((path, min(idx0, events[path]), s["event_list"].shape[1], fl, restarted, indices, float(s["dt_gt"])))
            out.append((jobs, flags[0], _state(ld), float(ld.last_proc_timestamp)))
        ld._end_pass()
    return out


def host_tables(probe, ts):
    """The index tables of a plan's boundary queries by the reference's own search on the files' timestamp columns."""
    return {p: np.asarray([binary_search_array(ts[p], q) for q in probe.queries[p]], dtype=np.int64) for p in probe.files}


@pytest.mark.parametrize("mode,window", CASES)
def test_plan_makes_h5loaders_decisions(tmp_path, mode, window):
    three_timed_files(tmp_path)
    cfg = _cfg(tmp_path, mode, window, B, RES, FLIPS)
    paths = [str(tmp_path / f"s{k}.npz") for k in range(3)]
    ts = {p: np.load(p)["events/ts"] for p in paths}
    events = {p: len(t) for p, t in ts.items()}
    _seed(1)
    ref = _Recording(cfg, 2, prefetch=0)
    ref.shuffle()
    want = h5_trajectory(ref, PASSES, events)
    assert any(r for _, r, _, _ in want)  # (a slot restarted)
    if mode == "time":
        assert any(j[0][2] != j[1][2] for j, _, _, _ in want)  # (two slots of one batch with different counts)

    probe = ResidentEvalPlan(cfg, 2)
    assert {p: m["events"] for p, m in probe.meta.items()} == events
    tables = host_tables(probe, ts)
    _seed(1)
    plan = ResidentEvalPlan(cfg, 2, meta=probe.meta, index=tables)
    plan.shuffle()
    n = 0
    for _ in range(PASSES):
        for jobs, (restarted, done) in plan.plan_batches():
            plan.new_seq, plan.pass_done = restarted, done  # (the loader's bookkeeping around a delivered batch)
            plan.samples += plan.batch_size
            w_jobs, w_restarted, w_state, w_last = want[n]
            assert jobs == w_jobs, (n, jobs, w_jobs)
            assert restarted == w_restarted and any(j[4] for j in jobs) == restarted, n
            assert _state(plan) == w_state, n
            path, row = plan.last_row
            assert float(ts[path][row] - probe.meta[path]["t0"]) == w_last, n
            n += 1
        plan._end_pass()
    assert n == len(want) and plan.epoch == PASSES


def test_windows_of_up_to_ten_events_are_empty(tmp_path):
    ts = gap_file(tmp_path / "gap.npz")
    cfg = _cfg(tmp_path, "time", 0.25, 1, RES)
    ref = H5Loader(cfg, 2, prefetch=0)
    plan = ResidentEvalPlan(cfg, 2)
    path = str(tmp_path / "gap.npz")
    counts = []
    for k in range(5):
        s = ref[k]
        _p, first, count, _fl, restarted, indices, dt_gt = plan.plan_sample(0)
        assert count == s["event_list"].shape[1] and not restarted and indices is None and dt_gt == 0.0
        counts.append(count)
        assert plan.last_row[0] == path and float(ts[plan.last_row[1]] - ts[0]) == float(ref.last_proc_timestamp), k
        if k in (2, 3):  # the five events of the third window were read, then dropped; the fourth window read nothing
            assert plan.last_row == (path, 604)
    assert counts[2] == counts[3] == 0 and min(counts[0], counts[1], counts[4]) > 10
    assert plan.batch_row == ref.batch_row


def test_refusals_come_before_any_device_work(tmp_path):
    (tmp_path / "maps").mkdir()
    (tmp_path / "bare").mkdir()
    _timed_sequence(tmp_path / "maps" / "a.npz", maps=1, frames=1)
    _timed_sequence(tmp_path / "bare" / "a.npz")
    for mode in ("gtflow_dt1", "frames"):
        with pytest.raises(_lib.EvflowError, match="H5Loader"):  # a map / frame that is not the loader resolution
            ResidentEvalLoader(_cfg(tmp_path / "maps", mode, 1, 1, (16, 24)), 2)
        with pytest.raises(_lib.EvflowError, match="H5Loader"):  # a file without the mode's group
            ResidentEvalLoader(_cfg(tmp_path / "bare", mode, 1, 1, RES), 2)
    with pytest.raises(_lib.EvflowError, match="ResidentLoader"):
        ResidentEvalLoader(_cfg(tmp_path / "maps", "events", 300, 1, RES), 2)
