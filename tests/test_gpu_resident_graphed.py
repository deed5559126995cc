"""Graph-replayed training on device-resident sequences (train.ResidentWindowStep, train_flow.py --graphed) on the MI355X, in
deterministic mode: the replayed steps -- whose sequence restarts zero-fill the recurrent state under a device flag -- against the
same launches run eagerly with `model.reset_states()`, bit for bit; the window buffers of a replay against the loader's
`next_window`; the driver with the replay on and off."""

import copy
import json
import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

from test_gpu_deterministic import LIF_NEURON, XLIF_NEURON, _model_cfg, cfg as loss_cfg
from test_gpu_head_det import PLIF_NEURON
from test_host_loader import _cfg
from test_host_resident import FLIPS, three_files

from event_flow_amd import _lib
from event_flow_amd.dataloader.resident import ResidentLoader
from event_flow_amd.loss.flow import EventWarping
from event_flow_amd.models.model import LIFFireNet, PLIFFireNet, XLIFFireNet
from event_flow_amd.train import FlatAdam, ResidentWindowStep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, N, P, PASSES, SEED = 2, 32, 40, 400, 3, 3, 9
LENGTHS = (4100, 3300, 2900)
NETS = {"lif": (LIFFireNet, LIF_NEURON), "plif": (PLIFFireNet, PLIF_NEURON), "xlif": (XLIFFireNet, XLIF_NEURON)}


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def _loader(path):
    np.random.seed(SEED)
    random.seed(SEED)
    ld = ResidentLoader(_cfg(path, "events", N, B, (H, W), FLIPS, hot=True), 2)
    ld.shuffle()
    return ld


def _run(path, kind, sd0, replay, after_step=None):
    """All optimizer steps of PASSES passes over the files -> (losses, state_dict, recurrent states, hot statistics, stats)."""
    cls, neuron = NETS[kind]
    model = cls(_model_cfg(neuron)).to(DEV)
    model.load_state_dict(sd0)
    model.train()
    assert model.compute_path[0] == "fused", model.compute_path
    opt = FlatAdam(model, lr=1e-3, clip=100.0, device_step=True)
    opt.zero_grad()
    ld = _loader(path)
    stepper = ResidentWindowStep(model, EventWarping(loss_cfg(H, W), DEV), opt, ld, P, warmup=2, replay=replay)
    losses = []
    for k, (discarded, group, reset, _epoch) in enumerate(ld.plan_steps(P, PASSES)):
        loss, info = stepper.step((discarded, group, reset))
        assert info["reset"] == reset and info["n_discarded"] == len(discarded) and len(info["done"]) == len(discarded) + P
        losses.append(loss.clone())  # (the next replay of the same graph rewrites the tensor)
        if after_step is not None:
            after_step(k, reset, stepper)
    torch.cuda.synchronize()
    out = (losses, copy.deepcopy(model.state_dict()), [s.clone() for s in model.states], (ld._hot_events.clone(), ld._hot_obvs.clone()),
           dict(stepper.stats))
    opt.close()
    return out


def _initial(kind):
    cls, neuron = NETS[kind]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh") or k.endswith("t0"):
                p.mul_(0.25)  # (an alive network: spikes in every layer, so that the state a restart clears is not zero anyway)
    return copy.deepcopy(first.state_dict())


@pytest.mark.parametrize("kind", sorted(NETS))
def test_replayed_steps_are_the_eager_steps(tmp_path, det_on, kind):
    three_files(tmp_path, H=H, W=W, lengths=LENGTHS)
    sd0 = _initial(kind)
    losses_r, sd_r, st_r, hot_r, stats = _run(tmp_path, kind, sd0, replay=True)
    losses_e, sd_e, st_e, hot_e, stats_e = _run(tmp_path, kind, sd0, replay=False)
    print(kind, "replayed run:", stats, "losses", [float(x) for x in losses_r])
    assert stats_e["replayed"] == 0 and stats_e["eager"] == len(losses_e) == len(losses_r)
    assert stats["eager"] == 2 and stats["replayed"] >= 6 and stats["replayed_reset"] >= 2
    assert stats["replayed"] - stats["replayed_reset"] >= 1 and stats["replayed_discarded"] >= 1
    assert stats["graph_a"] >= 1 and stats["graph_b"] >= 1 and stats["graph_a"] + stats["graph_b"] == stats["replayed"]
    assert all(np.isfinite(float(x)) and float(x) != 0 for x in losses_r)
    assert any(not torch.equal(sd0[k], sd_r[k]) for k in sd0)  # (it trained)
    assert any(float(s.abs().max()) > 0 for s in st_r)  # (a live state: zero-fill and drop are not trivially the same)
    for k, (a, b) in enumerate(zip(losses_r, losses_e)):
        assert torch.equal(a, b), (k, float(a), float(b))
    assert sd_r.keys() == sd_e.keys()
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_e[k]), (k, float((sd_r[k] - sd_e[k]).abs().max()))
    assert len(st_r) == len(st_e) == 7
    for i, (a, b) in enumerate(zip(st_r, st_e)):
        assert torch.equal(a, b), ("state of cell", i)
    assert torch.equal(hot_r[0], hot_e[0]) and torch.equal(hot_r[1], hot_e[1])


def test_replayed_window_buffers_are_next_windows(tmp_path, det_on):
    """After a replayed step with a restart and one without, the graph's static window buffers hold what a second loader's
    next_window(3) returns at the same step (same seed: the loaders are built one after the other, each from a fresh seed)."""
    three_files(tmp_path, H=H, W=W, lengths=LENGTHS)
    seen = {}

    def grab(k, reset, stepper):
        if k >= 2 and reset not in seen:
            assert stepper.stats["replayed"] == k - 1
            seen[reset] = (k, [{key: d[key].clone() for key in ("event_list", "event_cnt", "event_mask", "event_list_pol_mask")}
                               for d in stepper.passes])

    _run(tmp_path, "lif", _initial("lif"), replay=True, after_step=grab)
    assert set(seen) == {True, False}
    ld = _loader(tmp_path)
    windows = [ld.next_window(P) for _ in range(max(k for k, _ in seen.values()) + 1)]
    for reset, (k, got) in seen.items():
        passes, want_reset = windows[k]
        assert want_reset == reset
        for p in range(P):
            for key, t in got[p].items():
                assert t.shape == passes[p][key].shape and torch.equal(t, passes[p][key]), (k, p, key)


def test_driver_graphed_against_its_eager_windows(tmp_path, det_on, capsys):
    """train_flow.train --resident --graphed with the replay on and off: equal per-epoch losses, equal checkpoints, and the
    counters in the final JSON line."""
    import train_flow
    from event_flow_amd.configs.parser import YAMLParser

    (tmp_path / "data").mkdir()
    three_files(tmp_path / "data", H=H, W=W, lengths=LENGTHS)
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(train_flow.__file__)), "configs", "train_SNN.yml")))
    cfg["data"].update(path=str(tmp_path / "data"), window=400, window_loss=1200)
    cfg["loader"].update(batch_size=2, n_epochs=2, resolution=[32, 40], augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
    cfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    cfg["vis"]["verbose"] = False
    yaml.safe_dump(cfg, open(tmp_path / "train.yml", "w"))
    runs = []
    for replay in (True, False):
        out = str(tmp_path / f"m{int(replay)}.pth")
        args = types.SimpleNamespace(synthetic=False, prev="", out=out, epochs=3, fused_optimizer=True, resident=True, graphed=True)
        np.random.seed(9)
        random.seed(9)
        capsys.readouterr()
        history = train_flow.train(args, YAMLParser(str(tmp_path / "train.yml")), graphed_replay=replay)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        runs.append((copy.deepcopy(history), torch.load(out, map_location="cpu"), line))
    (h1, sd1, j1), (h0, sd0, j0) = runs
    assert len(h1) == 3 and all(np.isfinite(v) and v > 0 for v in h1), h1
    assert h1 == h0 and j1["loss_per_epoch"] == h1
    assert sd1.keys() == sd0.keys() and all(torch.equal(sd1[k], sd0[k]) for k in sd1)
    assert j1["graphed"]["replayed"] > 0 and j1["graphed"]["eager"] == 2
    assert j0["graphed"]["replayed"] == 0 and j0["graphed"]["eager"] == j1["graphed"]["eager"] + j1["graphed"]["replayed"]
