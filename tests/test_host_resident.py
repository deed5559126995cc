"""Host side of the device-resident loader (event_flow_amd/dataloader/resident.py) without a GPU: the cursor plan over
sequence lengths against what H5Loader's own host code (dataloader/h5.py:240-326) does on the same files, flags and RNG
state, the grouping of batches into training windows against a replay of train_flow.py's loop, and the refusals."""

import random

import numpy as np
import pytest

from test_host_loader import _cfg

from event_flow_amd import _lib
from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence
from event_flow_amd.dataloader.resident import ResidentLoader, ResidentPlan

WINDOW, B = 300, 2
LENGTHS = (1537, 1000, 700)
FLIPS = ("Horizontal", "Vertical", "Polarity")
EPOCHS = 6  # (two would do for the cursor; the window groups of P = 3 need more batches to show every case)


def three_files(path, H=16, W=20, seed=11, lengths=LENGTHS):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k, n in enumerate(lengths):
        ts = np.sort(rng.random(n)) * 2.0 + 50.0 * (k + 1)
        write_npz_sequence(str(path / f"s{k}.npz"), rng.integers(0, W, n), rng.integers(0, H, n), ts, rng.integers(0, 2, n))


class _Recording(H5Loader):
    """H5Loader that remembers which file every slot has open."""

    def _open(self, batch, path):
        self.__dict__.setdefault("paths", {})[batch] = path
        super()._open(batch, path)


def _state(ld):
    return (ld.new_seq, ld.pass_done, ld.seq_num, ld.epoch, ld.samples, tuple(ld.batch_idx), tuple(ld.batch_row))


def h5_trajectory(ld, epochs):
    """Per batch of `epochs` passes over the files: (jobs, restarted, state), jobs = (path, first, flags) per slot --
    `_host_batches` with the bookkeeping of `_deliver` (dataloader/h5.py:328-332), whose collate step needs the GPU."""
    out = []
    for _ in range(epochs):
        for samples, flags in ld._host_batches():
            assert all(s["event_list"].shape == (4, WINDOW) for s in samples)
            ld.new_seq, ld.pass_done = flags
            ld.samples += ld.batch_size
            jobs = [(ld.paths[b], ld.batch_row[b] - WINDOW, sum(bit for bit, m in zip((1, 2, 4), FLIPS) if ld.batch_augmentation[m][b]))
                    for b in range(ld.batch_size)]
            out.append((jobs, flags[0], _state(ld)))
        ld._end_pass()
    return out


def driver_groups(restarts, P):
    """train_flow.py:85-126 over the batches' `new_seq` flags: the optimizer steps once window_loss = P * window events are
    collected, a restart drops what was collected -> [(indices of the batches of a step, reset before the first)]."""
    groups, held, first_reset, num_events = [], [], False, 0
    for i, new_seq in enumerate(restarts):
        if new_seq:
            held, num_events = [], 0
        if not held:
            first_reset = new_seq
        held.append(i)
        num_events += WINDOW
        if num_events >= P * WINDOW:
            groups.append((held, first_reset))
            held, num_events = [], 0
    return groups


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_makes_h5loaders_decisions(tmp_path, seed):
    three_files(tmp_path)
    cfg = _cfg(tmp_path, "events", WINDOW, B, (16, 20), FLIPS)
    np.random.seed(seed)
    random.seed(seed)
    ref = _Recording(cfg, 2, prefetch=0)
    ref.shuffle()
    want = h5_trajectory(ref, EPOCHS)
    assert any(r for _, r, _ in want) and len({j[0][2] for j, _, _ in want} | {j[1][2] for j, _, _ in want}) > 1

    np.random.seed(seed)
    random.seed(seed)
    plan = ResidentPlan(cfg, 2)
    plan.shuffle()
    assert plan.lengths == {str(tmp_path / f"s{k}.npz"): n for k, n in enumerate(LENGTHS)}
    stream = plan._endless()
    for i, (jobs, restarted, state) in enumerate(want):
        got, got_restarted, _done = next(stream)
        assert [j[:3] for j in got] == jobs, i
        assert got_restarted == restarted and any(j[3] for j in got) == restarted, i
        assert _state(plan) == state, i
    assert plan.epoch == EPOCHS - 1 and next(stream) and plan.epoch == EPOCHS  # (the pass ends when the next one begins)

    # the windows of next_window(3) are the groups on which the training loop steps
    # (files this short restart a slot in most batches, so steps of P = 3 are rare; P = 2 shows the remaining cases)
    seen = {"groups": 0, "reset": 0, "dropped": 0}
    for P in (3, 2):
        np.random.seed(seed)
        random.seed(seed)
        plan = ResidentPlan(cfg, 2, lengths=plan.lengths)
        plan.shuffle()
        groups = driver_groups([r for _, r, _ in want], P)
        at = 0
        for idx, reset in groups:
            discarded, group, got_reset = plan.plan_window(P)
            assert got_reset == reset
            assert [[j[:3] for j in jobs] for jobs, _, _ in discarded] == [want[i][0] for i in range(at, idx[0])]
            assert [[j[:3] for j in jobs] for jobs, _, _ in group] == [want[i][0] for i in idx]
            at = idx[-1] + 1
            seen["groups"] += 1
            seen["reset"] += reset
            seen["dropped"] += len(discarded)
    assert seen["groups"] >= 3 and seen["reset"] and seen["dropped"], seen


def test_refusals_come_before_any_device_work(tmp_path):
    three_files(tmp_path)
    for mode, window in (("time", 0.25), ("events", 10)):
        with pytest.raises(_lib.EvflowError, match="H5Loader"):
            ResidentLoader(_cfg(tmp_path, mode, window, B, (16, 20)), 2)
    n = 800
    rng = np.random.Generator(np.random.PCG64(4))
    cols = dict(xs=rng.integers(0, 20, n), ys=rng.integers(0, 16, n), ps=rng.integers(0, 2, n))
    for name, bad, what in (("xs", 3.5, "events/xs"), ("ps", 2, "events/ps")):
        d = tmp_path / name
        d.mkdir()
        c = {k: v.astype(np.float64) if k == name else v for k, v in cols.items()}
        c[name][5] = bad
        for k in range(2):
            write_npz_sequence(str(d / f"s{k}.npz"), c["xs"], c["ys"], np.sort(rng.random(n)), c["ps"])
        with pytest.raises(_lib.EvflowError, match=what):
            ResidentLoader(_cfg(d, "events", WINDOW, B, (16, 20)), 2)
