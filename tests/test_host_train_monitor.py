"""Host side of the training monitor (event_flow_amd/monitor.py, utils/gradients.py, train_flow.py --monitor): the column names and
the row layout, the weight names against the reference-pickled checkpoint, the CSV writer, get_grads against numpy and every
refusal that comes before any device work.  No device."""

import csv
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_host_models import cfg as model_cfg

from event_flow_amd import _lib, monitor
from event_flow_amd.models import model as M
from event_flow_amd.utils.gradients import get_grads


def _weights(model):
    return [n for n, p in model.named_parameters() if "weight" in n]


@pytest.mark.parametrize("make,fused", [
    (lambda: M.LIFFireNet(model_cfg()), True),
    (lambda: M.PLIFFireNet(model_cfg(neuron={"leak_v": [-4.0, 0.1]})), True),
    (lambda: M.EVFlowNet(model_cfg(C=4, neuron=None, acts=("relu", None))), False),
])
def test_columns_and_row_layout(make, fused):
    model = make()
    assert (getattr(model, "compute_path", ("general", ""))[0] == "fused") == fused
    names = _weights(model)
    assert names and len(names) == len(set(names))
    cols = monitor.columns(model)
    assert cols[:3] == ["loss", "grad_norm", "clip_coef"]
    assert cols[3:3 + 3 * len(names)] == [f"{n}_{s}" for n in names for s in ("mean", "min", "max")]
    rates = cols[3 + 3 * len(names):]
    assert rates == ([f"rate/{layer}" for layer in ("1:head", "2:G1", "3:R1a", "4:R1b", "5:G2", "6:R2a", "7:R2b")] if fused else [])
    assert monitor.grad_columns(model) + monitor.rate_columns(model) == cols[3:]
    # the segments are the weights' places in a flat buffer of the trainable parameters in parameters() order
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad])
    params = dict(model.named_parameters())
    segs = monitor.weight_segments(model)
    assert [s[0] for s in segs] == names
    for name, off, n in segs:
        assert n == params[name].numel() and torch.equal(flat[off:off + n], params[name].detach().reshape(-1)), name


def test_frozen_parameters_have_no_columns():
    model = M.LIFFireNet(model_cfg())
    frozen = _weights(model)[1]
    dict(model.named_parameters())[frozen].requires_grad_(False)
    segs = monitor.weight_segments(model)
    assert frozen not in [s[0] for s in segs] and len(segs) == len(_weights(model)) - 1
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad])
    for name, off, n in segs:
        assert torch.equal(flat[off:off + n], dict(model.named_parameters())[name].detach().reshape(-1))


def test_weight_names_are_the_reference_checkpoints():
    """The columns of grads_w.csv carry the reference's parameter names: the key list of a checkpoint pickled by the reference."""
    g = load_golden("g14_checkpoint")
    reference = [k[len("param_"):] for k in g.files if k.startswith("param_") and "weight" in k]
    ours = _weights(M.LIFFireNet(model_cfg(C=8)))
    assert reference and sorted(reference) == sorted(ours)


def test_csv_writer_header_once_then_append(tmp_path):
    names = ["loss", "grad_norm", "clip_coef", "a.weight_mean", "a.weight_min", "a.weight_max", "rate/1:head", "rate/2:G1"]
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((5, len(names))).astype(np.float32)
    rows[1, 3], rows[2, 6], rows[3, 4] = np.float32(1e-40), np.float32(1) / np.float32(3), np.float32(np.inf)
    log = monitor.CsvLog(str(tmp_path / "out"), names)
    log.write(0, rows[:2])
    log.write(0, rows[2:3])  # (a drain in the middle of an epoch: the index goes on)
    log.write(1, rows[3:])
    log.write(1, rows[:0])
    again = monitor.CsvLog(str(tmp_path / "out"), names)  # a later run appends: no second header
    again.write(0, rows[:1])
    with open(tmp_path / "out" / "grads_w.csv", newline="") as f:
        grads = list(csv.reader(f))
    with open(tmp_path / "out" / "train_log.csv", newline="") as f:
        logs = list(csv.reader(f))
    assert grads[0] == ["", "a.weight_mean", "a.weight_min", "a.weight_max"]
    assert logs[0] == ["epoch", "step", "loss", "grad_norm", "clip_coef", "rate/1:head", "rate/2:G1"]
    assert len(grads) == len(logs) == 1 + 6 and all(r != grads[0] for r in grads[1:])
    assert [int(r[0]) for r in grads[1:]] == [0, 1, 2, 0, 1, 0]
    assert [(int(r[0]), int(r[1])) for r in logs[1:]] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (0, 0)]
    src = np.concatenate([rows, rows[:1]])
    back_g = np.array([[np.float32(v) for v in r[1:]] for r in grads[1:]], np.float32)
    back_l = np.array([[np.float32(v) for v in r[2:]] for r in logs[1:]], np.float32)
    assert np.array_equal(back_g.view(np.int32), src[:, 3:6].copy().view(np.int32))  # %.9g: a float32 survives the round trip
    assert np.array_equal(back_l.view(np.int32), src[:, [0, 1, 2, 6, 7]].copy().view(np.int32))
    # gradient columns only (the host path without the fused optimizer): no train_log.csv
    only = monitor.CsvLog(str(tmp_path / "host"), names[3:6])
    only.write(0, rows[:2, 3:6])
    assert (tmp_path / "host" / "grads_w.csv").exists() and not (tmp_path / "host" / "train_log.csv").exists()


def test_get_grads_against_numpy():
    torch.manual_seed(0)
    model = M.LIFFireNet(model_cfg(C=8))
    for p in model.parameters():
        p.grad = torch.randn_like(p) * 0.01
    skipped = _weights(model)[2]
    dict(model.named_parameters())[skipped].grad = None
    out = get_grads(model.named_parameters())
    names = [n for n in _weights(model) if n != skipped]
    assert list(out) == [f"{n}_{s}" for n in names for s in ("mean", "min", "max")]
    for n in names:
        g = np.abs(dict(model.named_parameters())[n].grad.numpy().astype(np.float64))
        assert abs(out[f"{n}_mean"] - g.mean()) <= 1e-6 * g.mean()
        assert out[f"{n}_min"] == g.min() and out[f"{n}_max"] == g.max()


def test_refusals_name_the_alternative(tmp_path, monkeypatch):
    import train_flow

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    model = M.LIFFireNet(model_cfg(C=8))
    with pytest.raises(_lib.EvflowError, match="FlatAdam") as e:
        monitor.TrainMonitor(model, torch.optim.Adam(model.parameters()))
    assert "--fused-optimizer" in str(e.value) and "get_grads" in str(e.value)
    assert monitor.refusal(fused_optimizer=True, want_rates=True) is None
    assert monitor.refusal(fused_optimizer=False, want_rates=False) is None  # vis.store_grads alone: served on the host
    why = monitor.refusal(fused_optimizer=False, want_rates=True)
    assert "--fused-optimizer" in why and "get_grads" in why
    monkeypatch.setenv("WORLD_SIZE", "2")
    why = monitor.refusal(fused_optimizer=True, want_rates=True)
    assert "WORLD_SIZE" in why and "data parallelism" in why and "WORLD_SIZE=1" in why
    with pytest.raises(_lib.EvflowError, match="data parallelism"):
        monitor.TrainMonitor(model, types.SimpleNamespace(flat_grad=None, norm_ws=None))
    monkeypatch.delenv("WORLD_SIZE")

    # the driver: refused after the configuration is read, before a loader, a model or an optimizer exists
    class Parser:
        device = "cpu"

        def __init__(self, store_grads):
            self.config = {"data": {"mode": "events"}, "vis": {"store_grads": store_grads}}

        def combine_entries(self, config):
            return config

    def args(**kw):
        return types.SimpleNamespace(**{**dict(synthetic=True, prev="", out="", epochs=1, fused_optimizer=True, resident=False,
                                               graphed=False, monitor=None), **kw})

    with pytest.raises(SystemExit, match="--fused-optimizer"):
        train_flow.train(args(monitor=str(tmp_path), fused_optimizer=False), Parser(False))
    monkeypatch.setenv("WORLD_SIZE", "2")
    for a, p in ((args(monitor=str(tmp_path)), Parser(False)), (args(), Parser(True))):
        with pytest.raises(SystemExit, match="data parallelism"):
            train_flow.train(a, p)
    monkeypatch.delenv("WORLD_SIZE")
    assert train_flow._monitor_dir(args(), Parser(False).config) is None
    assert train_flow._monitor_dir(args(), Parser(True).config) == "."
    assert train_flow._monitor_dir(args(out=str(tmp_path / "m.pth")), Parser(True).config) == str(tmp_path)
    assert train_flow._monitor_dir(args(monitor="logs", out=str(tmp_path / "m.pth")), Parser(True).config) == "logs"
    # a general-path model: the rate columns are missing, and the monitor says which path would have them
    general = M.EVFlowNet(model_cfg(C=4, neuron=None, acts=("relu", None)))
    assert monitor.rate_columns(general) == [] and not monitor.has_spike_rates(general)
    note = monitor.rates_notice(general)
    assert "general path" in note and "fused FireNet engine" in note and "log=True" in note
    assert monitor.rates_notice(M.LIFFireNet(model_cfg())) is None
