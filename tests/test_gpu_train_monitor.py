"""monitor.TrainMonitor on the MI355X, in deterministic mode: the monitor changes nothing about the steps it watches; its gradient
rows are the host get_grads on a clone of the flat gradient scaled by the logged clip coefficient; its spike rates are the counts
of `model(..., log=True)` on a second model; the rows logged by replayed graphs are those of the same launches run eagerly (with a
ring that wraps); the driver writes grads_w.csv / train_log.csv, byte-identical with the replay on and off."""

import copy
import csv
import json
import os
import random
import re
import types

import numpy as np
import pytest
import torch
import yaml

import train_log_ref as ref
from test_gpu_deterministic import LIF_NEURON, G, _model_cfg, cfg as loss_cfg
from test_gpu_head_det import PLIF_NEURON
from test_gpu_resident_graphed import LENGTHS, _initial, _loader
from test_host_resident import FLIPS, three_files

from event_flow_amd import _lib, synthetic
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.loss.flow import EventWarping
from event_flow_amd.models.model import LIFFireNet, PLIFFireNet
from event_flow_amd.monitor import HEAD, LAYERS, TrainMonitor
from event_flow_amd.train import FlatAdam, ResidentWindowStep, train_window, window_apply, window_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, N, P = 2, 32, 32, 400, 3
NETS = {"lif": (LIFFireNet, LIF_NEURON), "plif": (PLIFFireNet, PLIF_NEURON)}


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def _start(kind):
    """An alive network (thresholds scaled down: spikes in every layer) -> its state_dict."""
    cls, neuron = NETS[kind]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh"):
                p.mul_(0.25)
    return copy.deepcopy(first.state_dict())


def _model(kind, sd0, clip=100.0):
    cls, neuron = NETS[kind]
    m = cls(_model_cfg(neuron)).to(DEV)
    m.load_state_dict(sd0)
    m.train()
    assert m.compute_path[0] == "fused", m.compute_path
    opt = FlatAdam(m, lr=1e-3, clip=clip)
    opt.zero_grad()
    return m, opt, EventWarping(loss_cfg(H, W), DEV)


def _window(w):
    passes = [encode_event_list(G(synthetic.event_list_batch(B, N, H, W, 9100 + 100 * w + k)), 2, (H, W), want=("cnt", "mask", "pol"))
              for k in range(P)]
    for d in passes:
        d["event_voxel"] = None
    return passes


@pytest.mark.parametrize("kind", sorted(NETS))
def test_the_monitor_changes_nothing(det_on, kind):
    sd0 = _start(kind)
    runs = []
    for watched in (True, False):
        m, opt, lossf = _model(kind, sd0)
        mon = TrainMonitor(m, opt, rows=8) if watched else None
        start = opt.flat_param.clone()
        losses = [train_window(m, lossf, opt, _window(w), monitor=mon).clone() for w in range(4)]
        torch.cuda.synchronize()
        runs.append((opt.flat_param.clone(), opt.m.clone(), opt.v.clone(), losses, [s.clone() for s in m.states]))
        if watched:
            rows = mon.drain()
            assert rows.shape == (4, len(mon.columns())) and np.isfinite(rows).all()
            mon.close()
        opt.close()
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3])) and len(a[4]) == len(b[4]) == 7
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[4]))
    assert not torch.equal(a[0], start)  # (it trained)


@pytest.mark.parametrize("kind,clip", [("lif", 100.0), ("plif", 100.0), ("lif", 1e-3)])
def test_gradient_rows_are_get_grads_on_the_clipped_clone(det_on, kind, clip):
    m, opt, lossf = _model(kind, _start(kind), clip=clip)
    mon = TrainMonitor(m, opt, rows=8)
    cols = mon.columns()
    assert cols[:3] == list(HEAD) and cols[3] == mon.segments[0][0] + "_mean"
    clones, totals, losses = [], [], []
    for w in range(3):
        loss = window_backward(m, lossf, opt, _window(w), monitor=mon)
        clones.append(opt.flat_grad.clone())
        losses.append(window_apply(m, lossf, opt, loss, monitor=mon).clone())
        totals.append(opt.norm_ws[:1].clone())
    rows = mon.drain()
    assert rows.shape[0] == 3 and mon.pending == 0 and mon.drain().shape[0] == 0
    for w in range(3):
        row, g = rows[w], clones[w]
        assert float(g.abs().max()) > 0
        norm, coef = ref.clip_head(totals[w].cpu().numpy()[0], clip)
        assert ref.bits(row[0]) == ref.bits(losses[w].cpu().numpy()), (row[0], float(losses[w]))
        assert ref.bits(row[1]) == ref.bits(norm) and ref.bits(row[2]) == ref.bits(coef), (row[1:3], norm, coef)
        assert coef < 1 or clip >= 1  # (the tiny bound clips)
        for k, (name, off, n) in enumerate(mon.segments):
            scaled = (g[off:off + n] * float(row[2])).abs()  # get_grads on the clone scaled by the LOGGED coefficient
            mean64 = float(np.float64(row[2]) * g[off:off + n].double().abs().sum().item() / n)
            mean, mn, mx = row[3 + 3 * k:6 + 3 * k]
            print(f"step {w} {name}: mean {mean!r} (float64 {mean64!r}) min {mn!r} max {mx!r}")
            assert ref.bits(mn) == ref.bits(scaled.min().cpu().numpy()) and ref.bits(mx) == ref.bits(scaled.max().cpu().numpy()), name
            assert abs(float(mean) - mean64) <= ref.MEAN_RTOL * abs(mean64), (name, mean, mean64)
    mon.close()
    opt.close()


@pytest.mark.parametrize("kind", sorted(NETS))
def test_spike_rates_are_the_counts_of_log_true(det_on, kind):
    sd0 = _start(kind)
    m, opt, lossf = _model(kind, sd0)
    mon = TrainMonitor(m, opt, rows=8)
    cls, neuron = NETS[kind]
    twin = cls(_model_cfg(neuron)).to(DEV)
    twin.eval()
    bits_per_pass = B * H * W * 32
    assert bits_per_pass == 65536
    want = []
    for w in range(2):
        passes = _window(w)
        twin.load_state_dict(copy.deepcopy(m.state_dict()))
        twin.states = m.states  # (copies; None before the first window)
        counts = {layer: 0 for layer in LAYERS}
        with torch.no_grad():
            for d in passes:
                act = twin(d["event_voxel"], d["event_cnt"], log=True)["activity"]
                for layer in LAYERS:
                    c = act[layer] * bits_per_pass
                    assert abs(c - round(c)) < 1e-6
                    counts[layer] += int(round(c))
        want.append([ref.rate(counts[layer], P * bits_per_pass) for layer in LAYERS])
        train_window(m, lossf, opt, passes, monitor=mon)
    rows = mon.drain()
    off = mon.rate_offset
    assert mon.columns()[off:] == [f"rate/{layer}" for layer in LAYERS] and off + len(LAYERS) == rows.shape[1]
    print(kind, "rates", rows[:, off:].tolist())
    assert any(float(v) != 0 for step in want for v in step), "vacuous: no layer spikes"
    for w in range(2):
        assert np.array_equal(ref.bits(rows[w, off:]), ref.bits(np.array(want[w], np.float32))), (w, rows[w, off:], want[w])
    mon.close()
    opt.close()


def _resident_run(path, sd0, replay, rows):
    m = LIFFireNet(_model_cfg(LIF_NEURON)).to(DEV)
    m.load_state_dict(sd0)
    m.train()
    opt = FlatAdam(m, lr=1e-3, clip=100.0, device_step=True)
    opt.zero_grad()
    ld = _loader(path)
    mon = TrainMonitor(m, opt, rows=rows)
    stepper = ResidentWindowStep(m, EventWarping(loss_cfg(32, 40), DEV), opt, ld, 3, warmup=2, replay=replay, monitor=mon)
    logs, resets, drains = [], [], 0
    for k, (discarded, group, reset, _epoch) in enumerate(ld.plan_steps(3, 3)):
        if mon.full:
            logs.append(mon.drain())
            drains += 1
        stepper.step((discarded, group, reset))
        resets.append(reset)
    logs.append(mon.drain())
    out = (np.concatenate(logs), opt.flat_param.clone(), dict(stepper.stats), resets, drains)
    mon.close()
    opt.close()
    return out


@pytest.mark.parametrize("rows", [1024, 4])
def test_replayed_steps_log_what_the_eager_steps_log(tmp_path, det_on, rows):
    three_files(tmp_path, H=32, W=40, lengths=LENGTHS)
    sd0 = _initial("lif")
    log_r, par_r, stats, resets, drains = _resident_run(tmp_path, sd0, True, rows)
    log_e, par_e, stats_e, _resets, _drains = _resident_run(tmp_path, sd0, False, rows)
    steps = len(resets)
    assert steps >= 6 and any(resets[2:]) and stats["replayed"] == steps - 2 and stats["replayed_reset"] >= 1 and stats_e["replayed"] == 0
    assert drains == (0 if rows >= steps else (steps - 1) // rows)
    assert log_r.shape == log_e.shape and log_r.shape[0] == steps
    assert not np.isnan(log_r).any() and (log_r[:, 0] != 0).all()
    assert np.array_equal(log_r, log_e, equal_nan=True) and np.array_equal(ref.bits(log_r), ref.bits(log_e))
    assert torch.equal(par_r, par_e)


def _driver_cfg(tmp_path, resident, store_grads=False):
    import train_flow

    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(train_flow.__file__)), "configs", "train_SNN.yml")))
    cfg["data"].update(window=400, window_loss=1200)
    cfg["loader"].update(batch_size=2, n_epochs=2, resolution=[32, 40])
    if resident:
        (tmp_path / "data").mkdir()
        three_files(tmp_path / "data", H=32, W=40, lengths=LENGTHS)
        cfg["data"].update(path=str(tmp_path / "data"))
        cfg["loader"].update(augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
        cfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    cfg["vis"]["verbose"] = True
    if store_grads:
        cfg["vis"]["store_grads"] = True
    yaml.safe_dump(cfg, open(tmp_path / "train.yml", "w"))
    return str(tmp_path / "train.yml")


def _drive(capsys, yml, monitor, replay=True, **kw):
    import train_flow
    from event_flow_amd.configs.parser import YAMLParser

    args = types.SimpleNamespace(**{**dict(synthetic=False, prev="", out="", epochs=2, fused_optimizer=True, resident=False,
                                           graphed=False, monitor=monitor), **kw})
    np.random.seed(9)
    random.seed(9)
    capsys.readouterr()
    history = train_flow.train(args, YAMLParser(yml), graphed_replay=replay)
    out = capsys.readouterr().out
    steps = [int(s) for s in re.findall(r"\((\d+) optimizer steps", out)]
    return copy.deepcopy(history), steps, json.loads(out.strip().splitlines()[-1])


def _check_files(directory, steps):
    with open(os.path.join(directory, "grads_w.csv"), newline="") as f:
        grads = list(csv.reader(f))
    with open(os.path.join(directory, "train_log.csv"), newline="") as f:
        logs = list(csv.reader(f))
    names = [n for n, p in LIFFireNet(_model_cfg(LIF_NEURON)).named_parameters() if "weight" in n]
    assert grads[0] == [""] + [f"{n}_{s}" for n in names for s in ("mean", "min", "max")]
    assert logs[0] == ["epoch", "step"] + list(HEAD) + [f"rate/{layer}" for layer in LAYERS]
    assert len(grads) - 1 == len(logs) - 1 == sum(steps)
    index = [i for n in steps for i in range(n)]  # the step index restarts with every epoch
    assert [int(r[0]) for r in grads[1:]] == index and [int(r[1]) for r in logs[1:]] == index
    assert [int(r[0]) for r in logs[1:]] == [e for e, n in enumerate(steps) for _ in range(n)]
    values = np.array([[float(v) for v in r[1:]] for r in grads[1:]])
    assert np.isfinite(values).all() and (values >= 0).all() and values.max() > 0


def test_driver_synthetic_fused_optimizer(tmp_path, det_on, capsys):
    yml = _driver_cfg(tmp_path, resident=False)
    h_mon, steps, _line = _drive(capsys, yml, str(tmp_path / "mon"), synthetic=True)
    h_off, steps_off, _line = _drive(capsys, yml, None, synthetic=True)
    assert len(h_mon) == 2 and h_mon == h_off and steps == steps_off and min(steps) > 0
    _check_files(str(tmp_path / "mon"), steps)


def test_driver_store_grads_without_the_fused_optimizer(tmp_path, det_on, capsys):
    """vis.store_grads beside torch's Adam: get_grads on the host after clip_grad_norm_, into the directory of --out; no train_log."""
    yml = _driver_cfg(tmp_path, resident=False, store_grads=True)
    (tmp_path / "ck").mkdir()
    history, steps, _line = _drive(capsys, yml, None, synthetic=True, fused_optimizer=False, epochs=1, out=str(tmp_path / "ck" / "m.pth"))
    assert len(history) == 1 and len(steps) == 1 and steps[0] > 0
    with open(tmp_path / "ck" / "grads_w.csv", newline="") as f:
        grads = list(csv.reader(f))
    names = [n for n, p in LIFFireNet(_model_cfg(LIF_NEURON)).named_parameters() if "weight" in n]
    assert grads[0] == [""] + [f"{n}_{s}" for n in names for s in ("mean", "min", "max")]
    assert [int(r[0]) for r in grads[1:]] == list(range(steps[0]))
    values = np.array([[float(v) for v in r[1:]] for r in grads[1:]])
    assert np.isfinite(values).all() and (values >= 0).all() and values.max() > 0
    assert (values[:, 1::3] <= values[:, 0::3]).all() and (values[:, 0::3] <= values[:, 2::3]).all()  # min <= mean <= max
    assert not (tmp_path / "ck" / "train_log.csv").exists()


def test_driver_graphed_files_do_not_depend_on_the_replay(tmp_path, det_on, capsys):
    yml = _driver_cfg(tmp_path, resident=True)
    runs = [_drive(capsys, yml, str(tmp_path / f"mon{int(replay)}"), replay=replay, resident=True, graphed=True)
            for replay in (True, False)]
    h_off, steps_off, _line = _drive(capsys, yml, None, resident=True, graphed=True)
    (h1, steps1, j1), (h0, steps0, j0) = runs
    assert h1 == h0 == h_off and steps1 == steps0 == steps_off
    assert j1["graphed"]["replayed"] > 0 and j0["graphed"]["replayed"] == 0
    assert sum(steps1) == j1["graphed"]["eager"] + j1["graphed"]["replayed"]
    _check_files(str(tmp_path / "mon1"), steps1)
    for name in ("grads_w.csv", "train_log.csv"):
        assert open(tmp_path / "mon1" / name, "rb").read() == open(tmp_path / "mon0" / name, "rb").read(), name
