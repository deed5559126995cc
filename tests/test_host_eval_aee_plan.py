"""Host side of the graph-replayed AEE evaluation (ResidentEvalPlan.plan_eval_passes, evaluate.graphed_refusal,
eval_flow.py --resident --graphed in the ground-truth modes) without a GPU: the plan of passes against a direct walk of
H5Loader's own host code plus the evaluation loop's idx_AEE rule, the capacity of the replayed buffers, the draws from
np.random, and the refusals from arguments and configuration alone."""

import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

from test_host_eval_steps import _Fused, _General, _args
from test_host_loader import _cfg
from test_host_resident import FLIPS, _state
from test_host_resident_eval import RES, _Recording, h5_trajectory

from event_flow_amd import _lib
from event_flow_amd.dataloader.h5 import write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalPlan
from event_flow_amd.evaluate import graphed_refusal

CASES = [("gtflow_dt1", 1), ("gtflow_dt4", 0.25), ("gtflow_dt4", 0.5)]


def two_gt_files(path, H=RES[0], W=RES[1]):
    """a.npz: seven maps, the first two with the SAME stamp (the first window has dt_gt = 0 and no events: skipped, not
    counted), five events between the fourth and the fifth stamp (an empty window with dt_gt > 0: counted).  b.npz: five maps at
    an even pace."""
    rng = np.random.Generator(np.random.PCG64(21))
    out = {}
    for name, t0, stamps, gaps in (("a", 100.0, 100.0 + np.asarray([0.1, 0.1, 0.5, 0.9, 1.3, 1.7, 2.0]), ((100.9, 101.3),)),
                                   ("b", 300.0, 300.0 + 0.4 * np.arange(1, 6) + 0.01, ())):
        ts = t0 + np.sort(rng.random(2600)) * 2.1
        for lo, hi in gaps:
            ts = np.concatenate([ts[(ts < lo) | (ts >= hi)], lo + 0.05 * np.arange(1, 6)])
        ts = np.sort(ts)
        n = len(ts)
        groups = {g: [(f"{k:09d}", stamps[k], rng.standard_normal((2, H, W)).astype(np.float32)) for k in range(len(stamps))]
                  for g in ("flow_dt1", "flow_dt4")}
        write_npz_sequence(str(path / f"{name}.npz"), rng.integers(0, W, n), rng.integers(0, H, n), ts, rng.integers(0, 2, n), **groups)
        out[str(path / f"{name}.npz")] = n
    return out


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def loop_rule(walk, window):
    """eval_flow.py's idx_AEE statements over the batches the loop forwards: [(jobs, restarted, evaluate)]."""
    aee_every = int(np.round(1.0 / window))
    idx_AEE, out = 0, []
    for jobs, restarted in walk:
        evaluate = False
        if not float(jobs[0][6]) <= 0.0:
            idx_AEE += 1
            if idx_AEE == aee_every:
                evaluate, idx_AEE = True, 0
        out.append((jobs, restarted, evaluate))
    return out


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode,window", CASES)
def test_plan_eval_passes_is_the_loops_walk(tmp_path, mode, window, B):
    events = two_gt_files(tmp_path)
    cfg = _cfg(tmp_path, mode, window, B, RES, FLIPS)
    _seed(2)
    ref = _Recording(cfg, 2, prefetch=0)
    traj = h5_trajectory(ref, 1, events)
    drawn_ref = np.random.random()
    assert ref.pass_done and traj  # the last batch is the wrap-around one: the loop breaks on it before forwarding it
    want = loop_rule([(jobs, restarted) for jobs, restarted, _state_, _last in traj[:-1]], window)

    _seed(2)
    plan = ResidentEvalPlan(cfg, 2)
    got = list(plan.plan_eval_passes())
    drawn = np.random.random()
    assert got == want
    assert drawn == drawn_ref  # np.random was drawn from exactly as by iterating the loader
    assert _state(plan) == _state(ref) and plan.epoch == 1
    assert plan.batch_augmentation == ref.batch_augmentation

    counts = [job[2] for jobs, _r, _e in got for job in jobs]
    capacity = max(counts + [1])
    assert capacity == max(job[2] for jobs, _r, _s, _l in traj[:-1] for job in jobs) > 10
    evaluations = sum(1 for _j, _r, e in got if e)
    counted = sum(1 for jobs, _r, _e in got if jobs[0][6] > 0.0)
    assert evaluations == counted // int(np.round(1.0 / window)) >= 2
    assert any(r for _j, r, _e in got[1:])  # a sequence restart inside the run
    a = str(tmp_path / "a.npz")
    first_a = next(jobs for jobs, _r, _e in got if jobs[0][0] == a)
    first_a_eval = next(e for jobs, _r, e in got if jobs[0][0] == a)
    assert first_a[0][6] == 0.0 and first_a[0][2] == 0 and not first_a_eval  # dt_gt = 0: skipped, not counted
    assert any(job[2] == 0 and job[6] > 0.0 for jobs, _r, _e in got for job in jobs)  # an empty window that counts
    if B == 1 and window == 1:
        skipped = [i for i, (jobs, _r, _e) in enumerate(got) if not jobs[0][6] > 0.0]
        assert len(skipped) == 1 and [e for _j, _r, e in got] == [i not in skipped for i in range(len(got))]


def test_plan_eval_passes_refuses_the_other_modes(tmp_path):
    two_gt_files(tmp_path)
    plan = ResidentEvalPlan(_cfg(tmp_path, "time", 0.25, 1, RES), 2)
    with pytest.raises(_lib.EvflowError, match="ground-truth windows"):
        list(plan.plan_eval_passes())


def test_graphed_refusals_with_aee_need_no_device():
    cfg = {"data": {"mode": "gtflow_dt1", "window": 1, "window_eval": 1}, "metrics": {"name": ["AEE"]},
           "loss": {"overwrite_intermediate": False}}
    for mode in ("gtflow_dt1", "gtflow_dt4"):
        c = {**cfg, "data": {**cfg["data"], "mode": mode}}
        assert graphed_refusal(_args(), c) is None and graphed_refusal(_args(), c, _Fused()) is None
        assert graphed_refusal(_args(), {k: v for k, v in c.items() if k != "loss"}) is None
        why = graphed_refusal(_args(), c, _General())
        assert "general path" in why and "without --graphed" in why
        for names in (["AEE", "FWL"], ["FWL", "AEE"], ["AEE", "RSAT"], ["FWL", "RSAT"], []):
            why = graphed_refusal(_args(), {**c, "metrics": {"name": names}})
            assert mode in why and "ragged" in why and "AEE" in why and "without --graphed" in why, names
        why = graphed_refusal(_args(), {**c, "loss": {"overwrite_intermediate": True}})
        assert "overwrite_intermediate" in why and "--resident" in why and "without --graphed" in why and "ragged" not in why
        assert "--resident" in graphed_refusal(_args(resident=False), c)
        assert "--store" in graphed_refusal(_args(store="out"), c)
    for mode in ("time", "frames"):  # AEE alone does not open the other ragged modes
        why = graphed_refusal(_args(), {**cfg, "data": {**cfg["data"], "mode": mode}})
        assert mode in why and "ragged" in why and "without --graphed" in why
    why = graphed_refusal(_args(), {**cfg, "data": {"mode": "events", "window": 400, "window_eval": 1200}})
    assert why is not None and "AEE" in why and "drop --graphed" in why  # events mode with AEE: still refused
    why = graphed_refusal(_args(), {**cfg, "data": {"mode": "events", "window": 400, "window_eval": 1200},
                                    "metrics": {"name": ["FWL", "AEE"]}})
    assert why is not None and "drop --graphed" in why


def test_driver_refuses_graphed_aee_before_any_device_work(tmp_path, monkeypatch):
    """eval_flow.test itself in a ground-truth mode: the refusals are raised before a model is moved to the device or a
    loader is built, and the driver's own configuration asserts for AEE still fire."""
    import eval_flow
    from event_flow_amd.configs.parser import YAMLParser

    def no_device(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.nn.Module, "to", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    root = os.path.dirname(os.path.abspath(eval_flow.__file__))
    tcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_SNN.yml")))
    tcfg["loader"]["gpu"] = 0
    ecfg = yaml.safe_load(open(os.path.join(root, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(tmp_path), mode="gtflow_dt1", window=1, window_eval=1)
    ecfg["metrics"]["name"] = ["AEE"]

    def run(error, match, train=None, evalc=None):
        yaml.safe_dump(train or tcfg, open(tmp_path / "train.yml", "w"))
        yaml.safe_dump(evalc or ecfg, open(tmp_path / "eval.yml", "w"))
        args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", sequences=4, resident=True, graphed=True,
                                     synthetic=False, store="", per_sequence=False)
        with pytest.raises(error, match=match):
            eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")))

    run(_lib.EvflowError, "ragged", evalc={**ecfg, "metrics": {**ecfg["metrics"], "name": ["AEE", "FWL"]}})
    run(_lib.EvflowError, "overwrite_intermediate", evalc={**ecfg, "loss": {"overwrite_intermediate": True}})
    run(_lib.EvflowError, "drop --graphed", evalc={**ecfg, "data": {**ecfg["data"], "mode": "events", "window": 400, "window_eval": 1200}})
    ann = {k: v for k, v in tcfg.items() if k != "spiking_neuron"}  # the ANN FireNet: ConvLayer / ConvGRU cells
    ann["model"] = {**tcfg["model"], "name": "FireNet", "activations": ["relu", None]}
    run(_lib.EvflowError, "general path", train=ann)
