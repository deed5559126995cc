"""Graph-replayed AEE evaluation on ground-truth windows (evaluate.ResidentAEEStep, eval_flow.py --resident --graphed with
data.mode gtflow_dt1 / gtflow_dt4 and metrics [AEE]) on the MI355X, in deterministic mode (the voxel binning and the image of
warped events are order-dependent otherwise): a batch produced at capacity width against the loader's own batch, the replayed
passes -- whose sequence restarts zero-fill the recurrent state under a device word, whose AEE goes to a device log under a
row word that is -1 on a pass that does not evaluate -- against the same launches run eagerly, bit for bit, and the driver
against the eager loop on the resident loader and on H5Loader, per sequence file as well."""

import copy
import json
import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

import aee_at_ref as R
from test_gpu_eval_graphed import NETS, det_on  # noqa: F401  (det_on: fixture)
from test_host_loader import _cfg
from test_host_resident import FLIPS

from event_flow_amd import synthetic
from event_flow_amd.dataloader.h5 import write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader, ResidentEvalWindow
from event_flow_amd.evaluate import ResidentAEEStep
from test_gpu_deterministic import _model_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, SEED, SCALING = 32, 40, 9, 32
MODES = [("gtflow_dt1", 1), ("gtflow_dt4", 0.25)]


def two_files(path):
    """Two moving-dots sequences of about 4000 events: twelve flow_dt1 maps and five flow_dt4 maps in seq1, eight and four in
    seq0 (of two slots the first one restarts while the second still reads: a reset inside the run at B = 2 as well).  In BOTH files the
    first two stamps coincide -- the first window of a file has dt_gt = 0 and no events: the loop skips it without counting,
    and with two slots the first batch is all empty windows -- and seq1 has five events between two later stamps (an empty
    window that counts)."""
    for i in range(2):
        xs, ys, ts, ps, (u, v) = synthetic.moving_dots_events(4000, H, W, 40 + i, max_disp=20.0)
        ts = ts.astype(np.float64) * 1.25 + 5.0
        dt1 = 5.0 + 0.1 * np.asarray([1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11][:12 if i else 8], np.float64)
        dt4 = 5.0 + 0.25 * np.asarray([1, 1, 2, 3, 4][:5 if i else 4], np.float64)
        if i == 1:  # (between the stamps 5.5 and 5.6 of flow_dt1: inside the interval 5.5 .. 5.75 of flow_dt4)
            keep = (ts < 5.5) | (ts >= 5.6)
            xs, ys, ps = (np.concatenate([a[keep], a[~keep][:5]]) for a in (xs, ys, ps))
            ts = np.concatenate([ts[keep], 5.51 + 0.01 * np.arange(5)])
            order = np.argsort(ts, kind="stable")
            xs, ys, ts, ps = xs[order], ys[order], ts[order], ps[order]
        gt = np.zeros((2, H, W), np.float32)
        gt[0], gt[1] = u / 6, v / 6
        gt[:, ::5, ::3] = 0.0  # (pixels without ground truth)
        write_npz_sequence(str(path / f"seq{i}.npz"), xs.astype(np.int16), ys.astype(np.int16), ts, (ps > 0).astype(np.int8),
                           flow_dt1=[(f"{k:06d}", dt1[k], gt * (1 + 0.1 * k)) for k in range(len(dt1))],
                           flow_dt4=[(f"{k:06d}", dt4[k], gt * (2 + 0.3 * k)) for k in range(len(dt4))])


def _loader(path, mode, window, B, hot):
    np.random.seed(SEED)
    random.seed(SEED)
    return ResidentEvalLoader(_cfg(path, mode, window, B, (H, W), FLIPS, hot=hot), 2)


def _capacity(plan):
    return max([job[2] for jobs, _r, _e in plan for job in jobs] + [1])


# ------------------------------------------------------------------ capacity padding
@pytest.mark.parametrize("hot", [True, False])
@pytest.mark.parametrize("mode,window,B", [("gtflow_dt1", 1, 2), ("gtflow_dt4", 0.25, 1)])
def test_a_batch_at_capacity_width_is_the_loaders_batch(tmp_path, det_on, mode, window, B, hot):  # noqa: F811
    """Every batch of one pass over the files from `_produce` (width = the batch's own largest count) and from the static
    buffers at capacity width: bit-identical images, maps and doubles, the same rows in front, zero rows behind every count."""
    two_files(tmp_path)
    a, b = _loader(tmp_path, mode, window, B, hot), _loader(tmp_path, mode, window, B, hot)
    plan = list(a.plan_eval_passes())
    cap = _capacity(plan)
    win = ResidentEvalWindow(b, cap, extra_words=3)
    assert win.base == 2 * B + (5 * B + 1) // 2 and win.table_dev.numel() == win.base + 3
    widths = set()
    for k, (jobs, restarted, _e) in enumerate(plan):
        want = a._produce(jobs, restarted, False)
        extra = win.stage(jobs, k)
        extra[:] = -7
        win.send()
        got = win.launch()
        npad = max(j[2] for j in jobs)
        widths.add(npad)
        assert set(got) == set(want) and tuple(got["event_list"].shape) == (B, cap, 4) and tuple(want["event_list"].shape) == (B, npad, 4)
        for key in ("event_cnt", "event_voxel", "event_mask", "gtflow", "dt_input", "dt_gt"):
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and torch.equal(got[key], want[key]), (k, key)
        for key in ("event_list", "event_list_pol_mask"):
            assert torch.equal(got[key][:, :npad], want[key]), (k, key)
        for slot, job in enumerate(jobs):  # behind every slot's count: nothing
            assert not got["event_list"][slot, job[2]:].any() and not got["event_list_pol_mask"][slot, job[2]:].any(), (k, slot)
    assert 0 in widths and cap in widths and len(widths) > 3  # an all-empty batch, the widest one, ragged ones
    assert (win.table_dev[win.base:] == -7).all()
    if hot:
        assert torch.equal(a._hot_events, b._hot_events) and torch.equal(a._hot_obvs, b._hot_obvs) and int(a._hot_obvs.min()) > 0
    with pytest.raises(Exception, match="buffers of"):
        ResidentEvalWindow(b, cap - 1).stage(max((jobs for jobs, _r, _e in plan), key=lambda js: max(j[2] for j in js)), 0)


# ------------------------------------------------------------------ the stepper
def _initial(kind):
    cls, neuron = NETS[kind]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh") or k.endswith("t0"):
                p.mul_(0.25)  # (an alive network: spikes in every layer, so that the state a restart clears is not zero anyway)
    return copy.deepcopy(first.state_dict())


def _run(path, kind, sd0, mode, window, B, hot, replay):
    cls, neuron = NETS[kind]
    model = cls(_model_cfg(neuron)).to(DEV)
    model.load_state_dict(sd0)
    model.eval()
    assert model.compute_path[0] == "fused", model.compute_path
    ld = _loader(path, mode, window, B, hot)
    plan = list(ld.plan_eval_passes())
    evals = sum(1 for _j, _r, e in plan if e)
    stepper = ResidentAEEStep(model, ld, len(plan), evals, _capacity(plan), SCALING, warmup=2, replay=replay, per_sequence=True)
    model.reset_states()
    live = 0
    for k, (jobs, restarted, evaluate) in enumerate(plan):
        if k >= 2 and restarted:  # (a test's read; the stepper itself reads nothing)
            live += any(float(s.abs().max()) > 0 for s in model.states)
        stepper.step(jobs, restarted, evaluate)
    out = stepper.results()
    torch.cuda.synchronize()
    hot_stats = (ld._hot_events.clone(), ld._hot_obvs.clone()) if hot else ()
    return (stepper.aee_log.clone(), stepper.sharp_log.clone(), out, [s.clone() for s in model.states], hot_stats, dict(stepper.stats),
            live, stepper.row_files, plan)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode,window", MODES)
@pytest.mark.parametrize("kind", ["lif", "plif"])
def test_replayed_passes_are_the_eager_passes(tmp_path, det_on, kind, mode, window, B):  # noqa: F811
    two_files(tmp_path)
    hot = (B == 1) == (mode == "gtflow_dt1")  # the filter on and off, in both modes and batch sizes
    sd0 = _initial(kind)
    aee_r, sharp_r, out_r, st_r, hot_r, stats, live, files, plan = _run(tmp_path, kind, sd0, mode, window, B, hot, True)
    aee_e, sharp_e, out_e, st_e, hot_e, stats_e, _l, files_e, _p = _run(tmp_path, kind, sd0, mode, window, B, hot, False)
    n, evals = len(plan), sum(1 for _j, _r, e in plan if e)
    print(kind, mode, B, "passes", n, "evaluations", evals, stats, {k: v for k, v in out_r.items() if k != "per_sequence"})
    assert not plan[0][2] and plan[0][0][0][6] == 0.0  # the first pass is skipped (dt_gt = 0): its AEE row word is -1
    assert sum(1 for _j, _r, e in plan[2:] if e) >= 2 and any(not e for _j, _r, e in plan[2:])  # replayed: evaluated and not
    assert stats_e == {"eager": n, "replayed": 0, "replayed_reset": 0, "graph_a": 0, "graph_b": 0}
    assert stats["eager"] == 2 and stats["replayed"] == n - 2 and stats["graph_a"] >= 1 and stats["graph_b"] >= 1
    assert stats["graph_a"] + stats["graph_b"] == stats["replayed"]
    assert stats["replayed_reset"] == sum(1 for _j, r, _e in plan[2:] if r) >= 1 and stats["replayed"] > stats["replayed_reset"]
    assert live >= 1  # a live state in front of a replayed reset: zero-fill and drop are not trivially the same
    assert tuple(aee_r.shape) == (evals, 2 * (B + 1)) and tuple(sharp_r.shape) == (n,)
    assert not torch.isnan(aee_r).any() and not torch.isnan(sharp_r).any()
    means = aee_r[:, B].tolist()  # (0: the evaluated window without events -- no valid pixel, 0 / 1e-9)
    assert min(means) >= 0 and sum(1 for v in means if v > 0) >= evals - 1 and len(set(means)) == evals
    # bit for bit
    assert torch.equal(aee_r, aee_e) and torch.equal(sharp_r, sharp_e)
    assert len(st_r) == len(st_e) == 7 and any(float(s.abs().max()) > 0 for s in st_r)
    for i, (x, y) in enumerate(zip(st_r, st_e)):
        assert torch.equal(x, y), ("state of cell", i)
    for x, y in zip(hot_r, hot_e):
        assert torch.equal(x, y)
    assert files == files_e and len(files) == evals and {f for row in files for f in row} == {"seq0.npz", "seq1.npz"}
    assert out_r == out_e
    host = aee_r.cpu().tolist()
    assert out_r["AEE"] == sum(row[B] for row in host) / evals and out_r["AEE_percent_outliers"] == sum(row[-1] for row in host) / evals
    assert out_r["iwe_variance"] == float(sharp_r.mean())
    assert sum(v["it"] for v in out_r["per_sequence"].values()) == evals * B


# ------------------------------------------------------------------ the driver
@pytest.mark.parametrize("B", [1, 2])
def test_driver_graphed_aee_against_the_eager_loops(tmp_path, det_on, capsys, B):  # noqa: F811
    """eval_flow.test --resident --graphed --per-sequence, --resident --per-sequence and plain H5Loader --per-sequence in
    gtflow_dt1 with metrics [AEE]: iwe_variance and the outlier percentage equal (the flows and the counts are identical, a
    mean of at most two elements does not depend on the order), AEE within the summation bound of evf_aee_at (tests/
    aee_at_ref.py), in total and per file; the same number of evaluations."""
    import eval_flow
    from event_flow_amd.configs.parser import YAMLParser

    (tmp_path / "data").mkdir()
    two_files(tmp_path / "data")
    root = os.path.dirname(os.path.abspath(eval_flow.__file__))
    tcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    tcfg["loader"].update(resolution=[H, W])
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    ecfg = yaml.safe_load(open(os.path.join(root, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path / "data"), mode="gtflow_dt1", window=1, window_eval=1)
    ecfg["loader"].update(batch_size=B, resolution=[H, W], augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
    ecfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    ecfg["metrics"]["name"] = ["AEE"]
    ecfg["metrics"]["flow_scaling"] = SCALING
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))

    def run(resident, graphed, replay=True):
        torch.manual_seed(4)
        np.random.seed(SEED)
        random.seed(SEED)
        args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", synthetic=False, sequences=4,
                                     resident=resident, store="", graphed=graphed, per_sequence=True)
        capsys.readouterr()
        out = eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")), graphed_replay=replay)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
        return out

    g1, res, h5 = run(True, True), run(True, False), run(False, False)
    today = {"model", "iwe_variance", "AEE", "AEE_percent_outliers", "per_sequence"}
    assert set(h5) == set(res) == today and set(g1) == today | {"graphed"}
    st = g1["graphed"]
    assert st["eager"] == 2 and st["replayed"] == st["passes"] - 2 and st["graph_a"] >= 1 and st["graph_b"] >= 1 and st["replayed_reset"] >= 1
    assert st["evaluations"] >= 3 and st["passes"] > st["evaluations"]
    bound = R.bound(H, W)
    assert np.isfinite(g1["AEE"]) and g1["AEE"] > 0 and g1["iwe_variance"] > 0 and 0 < g1["AEE_percent_outliers"]
    for name, other in (("--resident", res), ("H5Loader", h5)):
        print(name, {k: (g1[k], other[k]) for k in ("iwe_variance", "AEE", "AEE_percent_outliers")}, "bound", bound)
        assert g1["model"] == other["model"]
        assert g1["iwe_variance"] == other["iwe_variance"], name
        assert g1["AEE_percent_outliers"] == other["AEE_percent_outliers"], name
        assert abs(g1["AEE"] - other["AEE"]) <= bound * other["AEE"], name
        assert set(g1["per_sequence"]) == set(other["per_sequence"]) == {"seq0.npz", "seq1.npz"}
        for f, mine in g1["per_sequence"].items():
            theirs = other["per_sequence"][f]
            assert set(mine) == set(theirs) == {"AEE", "AEE_percent_outliers", "it"} and mine["it"] == theirs["it"], (name, f)
            assert mine["AEE_percent_outliers"] == theirs["AEE_percent_outliers"], (name, f)
            assert abs(mine["AEE"] - theirs["AEE"]) <= bound * theirs["AEE"], (name, f)
    # the number of evaluations: every slot's value of every evaluation went to one file
    assert sum(v["it"] for v in g1["per_sequence"].values()) == st["evaluations"] * B
    assert sum(v["it"] for v in res["per_sequence"].values()) == st["evaluations"] * B
