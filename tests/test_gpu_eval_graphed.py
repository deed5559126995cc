"""Graph-replayed evaluation on device-resident sequences (evaluate.ResidentEvalStep, eval_flow.py --resident --graphed) on the
MI355X, in deterministic mode (RSAT's float splats are order-dependent otherwise): the replayed windows -- whose sequence
restarts zero-fill the recurrent state under a device word per pass, and whose results go to a device log -- against the same
launches run eagerly with `model.reset_states()`, bit for bit; the driver with the replay on and off against the eager loop on
the resident loader and on H5Loader, per sequence file as well."""

import copy
import random
import types

import numpy as np
import pytest
import torch
import yaml

from test_gpu_deterministic import LIF_NEURON, XLIF_NEURON, _model_cfg
from test_gpu_head_det import PLIF_NEURON
from test_host_eval_steps import B, H, LENGTHS, N, SEED, W
from test_host_loader import _cfg
from test_host_resident import FLIPS, three_files

from event_flow_amd import _lib
from event_flow_amd.dataloader.resident import ResidentLoader
from event_flow_amd.evaluate import ResidentEvalStep, reduce_eval_log, row_layout
from event_flow_amd.loss.flow import FWL, RSAT
from event_flow_amd.models.model import LIFFireNet, PLIFFireNet, XLIFFireNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["FWL", "RSAT"]
SCALING = 64
NETS = {"lif": (LIFFireNet, LIF_NEURON), "plif": (PLIFFireNet, PLIF_NEURON), "xlif": (XLIFFireNet, XLIF_NEURON)}


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def _initial(kind):
    cls, neuron = NETS[kind]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh") or k.endswith("t0"):
                p.mul_(0.25)  # (an alive network: spikes in every layer, so that the state a restart clears is not zero anyway)
    return copy.deepcopy(first.state_dict())


def _run(path, kind, sd0, replay, P):
    """One pass over the files -> (log, results, recurrent states, hot statistics, counters, windows found with a live state
    in front of a reset)."""
    cls, neuron = NETS[kind]
    model = cls(_model_cfg(neuron)).to(DEV)
    model.load_state_dict(sd0)
    model.eval()
    assert model.compute_path[0] == "fused", model.compute_path
    config = {"loader": {"resolution": [H, W]}, "loss": {"overwrite_intermediate": False}}
    criteria = [FWL(config, DEV, flow_scaling=SCALING), RSAT(config, DEV, flow_scaling=SCALING)]
    np.random.seed(SEED)
    random.seed(SEED)
    ld = ResidentLoader(_cfg(path, "events", N, B, (H, W), FLIPS, hot=True), 2)
    steps = list(ld.plan_eval_steps(P))
    stepper = ResidentEvalStep(model, criteria, NAMES, ld, P, len(steps) - 1, SCALING, warmup=2, replay=replay, per_sequence=True)
    live = 0
    for k, (group, pass_reset, tail) in enumerate(steps):
        if tail:
            stepper.step_tail(group, pass_reset)
            continue
        if k >= 2 and pass_reset[0]:  # (a test's read; the stepper itself reads nothing)
            live += any(float(s.abs().max()) > 0 for s in model.states)
        stepper.step(group, pass_reset)
    out = stepper.results()
    torch.cuda.synchronize()
    tail = torch.stack(stepper.tail_sharp) if stepper.tail_sharp else torch.empty(0, device=DEV)
    return (stepper.log.clone(), tail.clone(), out, [s.clone() for s in model.states], (ld._hot_events.clone(), ld._hot_obvs.clone()),
            dict(stepper.stats), live, stepper.row_files, [r for _g, r, t in steps if not t])


@pytest.mark.parametrize("P", [3, 1])
@pytest.mark.parametrize("kind", sorted(NETS))
def test_replayed_windows_are_the_eager_windows(tmp_path, det_on, kind, P):
    three_files(tmp_path, H=H, W=W, lengths=LENGTHS)
    sd0 = _initial(kind)
    log_r, tail_r, out_r, st_r, hot_r, stats, live, files, resets = _run(tmp_path, kind, sd0, True, P)
    log_e, tail_e, out_e, st_e, hot_e, stats_e, _live, files_e, _resets = _run(tmp_path, kind, sd0, False, P)
    print(kind, P, "replayed run:", stats, {k: v for k, v in out_r.items() if k != "per_sequence"})
    rows = 35 // P
    assert tuple(log_r.shape) == (rows, row_layout(2, B, P)) and not torch.isnan(log_r).any() and not torch.isinf(log_r).any()
    assert stats_e == {"eager": rows, "replayed": 0, "replayed_reset": 0, "graph_a": 0, "graph_b": 0, "tail_passes": 35 % P}
    assert stats["eager"] == 2 and stats["replayed"] == rows - 2 and stats["tail_passes"] == 35 % P
    assert stats["graph_a"] >= 1 and stats["graph_b"] >= 1 and stats["graph_a"] + stats["graph_b"] == stats["replayed"]
    replayed = resets[2:]
    assert stats["replayed_reset"] == sum(1 for r in replayed if any(r)) >= 2
    assert stats["replayed"] - stats["replayed_reset"] >= 1  # a replay that must leave the state alone
    if P == 3:
        assert any(r[0] for r in replayed) and any(not r[0] and any(r[1:]) for r in replayed)  # a reset at a pass > 0, too
    assert live >= 1  # a live state in front of a replayed reset: zero-fill and drop are not trivially the same
    assert float(log_r[:, :2 * (B + 1)].abs().min()) > 0 and len({float(v) for v in log_r[:, B]}) == rows  # (FWL differs per window)
    # bit for bit
    assert torch.equal(log_r, log_e) and torch.equal(tail_r, tail_e)
    assert len(st_r) == len(st_e) == 7 and any(float(s.abs().max()) > 0 for s in st_r)
    for i, (a, b) in enumerate(zip(st_r, st_e)):
        assert torch.equal(a, b), ("state of cell", i)
    assert torch.equal(hot_r[0], hot_e[0]) and torch.equal(hot_r[1], hot_e[1])
    assert files == files_e and len(files) == rows and len({f for row in files for f in row}) == 3
    assert out_r == out_e == reduce_eval_log(log_e, tail_e, NAMES, B, P, files)
    assert set(out_r["per_sequence"]) == {"s0.npz", "s1.npz", "s2.npz"}
    assert sum(v["it"] for v in out_r["per_sequence"].values()) == rows * B


def test_driver_graphed_against_the_eager_loops(tmp_path, det_on, capsys):
    """eval_flow.test --resident --graphed --per-sequence with the replay on and off, --resident --per-sequence and plain
    H5Loader --per-sequence: the same numbers, key by key and file by file."""
    import json
    import os

    import eval_flow
    from event_flow_amd.configs.parser import YAMLParser

    (tmp_path / "data").mkdir()
    three_files(tmp_path / "data", H=H, W=W, lengths=LENGTHS)
    root = os.path.dirname(os.path.abspath(eval_flow.__file__))
    tcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    tcfg["loader"].update(resolution=[H, W])
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    ecfg = yaml.safe_load(open(os.path.join(root, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path / "data"), mode="events", window=N, window_eval=3 * N)
    ecfg["loader"].update(batch_size=B, resolution=[H, W], augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
    ecfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    ecfg["metrics"]["name"] = list(NAMES)
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))

    def run(resident, graphed, per_sequence, replay=True):
        torch.manual_seed(4)
        np.random.seed(SEED)
        random.seed(SEED)
        args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", synthetic=False, sequences=4,
                                     resident=resident, store="", graphed=graphed, per_sequence=per_sequence)
        capsys.readouterr()
        out = eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")), graphed_replay=replay)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
        return out

    g1, g0 = run(True, True, True), run(True, True, True, replay=False)
    res, h5 = run(True, False, True), run(False, False, True)
    today = {"model", "iwe_variance", "FWL", "RSAT"}
    assert set(h5) == set(res) == today | {"per_sequence"} and set(g1) == set(g0) == today | {"per_sequence", "graphed"}
    assert g1["graphed"] == {"eager": 2, "replayed": 9, "replayed_reset": 2, "graph_a": 5, "graph_b": 4, "tail_passes": 2}
    assert g0["graphed"] == {"eager": 11, "replayed": 0, "replayed_reset": 0, "graph_a": 0, "graph_b": 0, "tail_passes": 2}
    for name, other in (("replay off", g0), ("--resident", res), ("H5Loader", h5)):
        for key in ("model", "iwe_variance", "FWL", "RSAT"):
            print(name, key, g1[key], other[key])
            assert g1[key] == other[key], (name, key, g1[key], other[key])
        assert g1["per_sequence"] == other["per_sequence"], name
    assert np.isfinite(g1["FWL"]) and g1["FWL"] > 0 and np.isfinite(g1["RSAT"]) and g1["RSAT"] > 0 and g1["iwe_variance"] > 0
    assert set(g1["per_sequence"]) == {"s0.npz", "s1.npz", "s2.npz"}
    assert all(set(v) == {"FWL", "RSAT", "it"} for v in g1["per_sequence"].values())
    assert sum(v["it"] for v in g1["per_sequence"].values()) == 11 * B
    # without --per-sequence the key set is today's (+ the counters of --graphed)
    assert set(run(True, True, False)) == today | {"graphed"} and set(run(True, False, False)) == today
