"""Host side of the graph-replayed evaluation (event_flow_amd/evaluate.py, eval_flow.py --graphed) without a GPU: the plan of
evaluated windows against a direct walk of the loader's batches, the refusals of --graphed from arguments and configuration
alone, and the reduction of the result log against the eager loop's accumulation."""

import random
import types

import numpy as np
import pytest
import torch

from test_host_loader import _cfg
from test_host_resident import FLIPS, three_files

from event_flow_amd import _lib
from event_flow_amd.dataloader.resident import ResidentPlan
from event_flow_amd.evaluate import PerSequence, graphed_refusal, reduce_eval_log, row_layout

B, H, W, N, SEED = 2, 32, 40, 400, 9
LENGTHS = (9100, 7300, 6900)  # (tests/test_gpu_eval_graphed.py evaluates these files)


def eval_plan(path):
    np.random.seed(SEED)
    random.seed(SEED)
    lengths = {str(path / f"s{k}.npz"): n for k, n in enumerate(LENGTHS)}
    return ResidentPlan(_cfg(path, "events", N, B, (H, W), FLIPS, hot=True), 2, lengths=lengths)  # (no shuffle)


@pytest.mark.parametrize("P", [1, 3])
def test_plan_eval_steps_groups_the_batches_before_the_wrap_around(tmp_path, P):
    three_files(tmp_path, H=H, W=W, lengths=LENGTHS)
    walk = []
    ref = eval_plan(tmp_path)
    for jobs, (restarted, done) in ref.plan_batches():
        if done:
            break
        walk.append((jobs, restarted))
    ref._end_pass()
    assert len(walk) == 35 and not walk[0][1] and any(r for _, r in walk)

    plan = eval_plan(tmp_path)
    steps = list(plan.plan_eval_steps(P))
    assert [t for _g, _r, t in steps] == [False] * (len(walk) // P) + [True]
    got = [batch for group, _r, _t in steps for batch in group]
    assert [(jobs, restarted) for jobs, restarted, _done in got] == walk and not any(done for _j, _r, done in got)
    for group, pass_reset, tail in steps:
        assert pass_reset == [restarted for _j, restarted, _d in group]
        assert len(group) == (len(walk) % P if tail else P)
    # one pass over the files, with the bookkeeping of the loader's own iteration
    assert (plan.epoch, plan.seq_num, plan.samples, plan.new_seq) == (ref.epoch, ref.seq_num, B * (len(walk) + 1), False)
    assert plan.batch_idx == ref.batch_idx and plan.batch_row == ref.batch_row
    if P == 3:
        # what tests/test_gpu_eval_graphed.py replays after its two eager steps: every case of a restart
        assert len(steps) == 12 and len(steps[-1][0]) == 2
        replayed = [r for _g, r, _t in steps[2:-1]]
        assert len(replayed) == 9
        assert sum(1 for r in replayed if r[0]) == 1                      # the state of the previous graph is cleared
        assert sum(1 for r in replayed if not r[0] and any(r[1:])) == 1   # ... the state pass p - 1 of the same graph wrote
        assert sum(1 for r in replayed if not any(r)) == 7


def test_plan_eval_steps_leaves_the_training_plan_alone(tmp_path):
    three_files(tmp_path, H=H, W=W, lengths=LENGTHS)
    a, b = eval_plan(tmp_path), eval_plan(tmp_path)
    list(b.plan_eval_steps(3))
    assert b._stream is None
    np.random.seed(SEED)
    fresh = [a.plan_window(3) for _ in range(4)]
    c = eval_plan(tmp_path)
    np.random.seed(SEED)
    assert [c.plan_window(3) for _ in range(4)] == fresh
    with pytest.raises(_lib.EvflowError, match="groups of 0"):
        list(a.plan_eval_steps(0))


class _Fused:
    compute_path = ("fused", "")


class _General:
    compute_path = ("general", "cell kind(s) ConvGRU")


def _args(**kw):
    base = dict(resident=True, graphed=True, synthetic=False, store="", per_sequence=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_graphed_refusals_need_no_device(tmp_path):
    cfg = {"data": {"mode": "events", "window": 400, "window_eval": 1200}, "metrics": {"name": ["FWL", "RSAT"]}}
    assert graphed_refusal(_args(), cfg) is None and graphed_refusal(_args(), cfg, _Fused()) is None
    assert "--resident" in graphed_refusal(_args(resident=False), cfg)
    assert "--synthetic" in graphed_refusal(_args(synthetic=True), cfg)
    assert "--store" in graphed_refusal(_args(store="out"), cfg)
    for mode in ("time", "frames", "gtflow_dt1", "gtflow_dt4"):
        why = graphed_refusal(_args(), {**cfg, "data": {**cfg["data"], "mode": mode}})
        assert mode in why and "ragged" in why and "AEE" in why and "without --graphed" in why
    why = graphed_refusal(_args(), cfg, _General())
    assert "general path" in why and "ConvGRU" in why and "without --graphed" in why
    assert graphed_refusal(types.SimpleNamespace(resident=True), cfg) is None  # (hand-made args without the newer flags)


def test_driver_refuses_graphed_before_any_device_work(tmp_path, monkeypatch):
    """eval_flow.test itself: every refusal is raised before a model is moved to the device or a loader is built."""
    import os

    import yaml

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
    ecfg["data"].update(path=str(tmp_path), mode="events", window=400, window_eval=1200)
    ecfg["metrics"]["name"] = ["FWL", "RSAT"]

    def run(match, train=None, evalc=None, **kw):
        yaml.safe_dump(train or tcfg, open(tmp_path / "train.yml", "w"))
        yaml.safe_dump(evalc or ecfg, open(tmp_path / "eval.yml", "w"))
        args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", sequences=4,
                                     **{**dict(resident=True, graphed=True, synthetic=False, store=""), **kw})
        with pytest.raises(_lib.EvflowError, match=match):
            eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")))

    run("add --resident", resident=False)
    run("drop --synthetic", synthetic=True)
    run("use --store", store=str(tmp_path / "png"))
    run("'time'", evalc={**ecfg, "data": {**ecfg["data"], "mode": "time", "window": 0.25}})
    ann = {k: v for k, v in tcfg.items() if k != "spiking_neuron"}  # the ANN FireNet: ConvLayer / ConvGRU cells
    ann["model"] = {**tcfg["model"], "name": "FireNet", "activations": ["relu", None]}
    run("general path", train=ann)


def test_log_reduction_is_the_eager_accumulation():
    """A hand-made log of 5 windows, K = 2, B = 2, P = 3, two tail passes, the two slots on different files that change on the
    way: against the eager loop's own statements (eval_flow.py: `+= float(val.mean())`, `/ max(it, 1)`,
    `torch.stack(iwe_sharpness).mean()`) and the reference's per-file sums."""
    names, K, P, rows = ["FWL", "RSAT"], 2, 3, 5
    g = torch.Generator().manual_seed(5)
    vals = torch.rand((rows, K, B), generator=g, dtype=torch.float32) * 3 + 0.1
    sharp = torch.rand((rows, P), generator=g, dtype=torch.float32) * 7
    tail = torch.rand(2, generator=g, dtype=torch.float32)
    log = torch.full((rows, row_layout(K, B, P)), float("nan"))
    files = [["a.npz", "b.npz"], ["a.npz", "b.npz"], ["a.npz", "c.npz"], ["a.npz", "c.npz"], ["b.npz", "c.npz"]]
    results = {m: {"metric": 0.0, "it": 0} for m in names}
    iwe_sharpness, per = [], {}
    for r in range(rows):
        for p in range(P):
            iwe_sharpness.append(sharp[r, p].clone())
        for k, name in enumerate(names):
            val = vals[r, k]
            log[r, k * (B + 1):k * (B + 1) + B] = val
            log[r, k * (B + 1) + B] = val.mean()
            results[name]["it"] += 1
            results[name]["metric"] += float(val.mean())
            for b in range(B):  # (reference eval_flow.py:183-199)
                cell = per.setdefault(files[r][b], {}).setdefault(name, {"metric": 0.0, "it": 0})
                cell["it"] += 1
                cell["metric"] += float(val[b])
        log[r, K * (B + 1):] = sharp[r]
    iwe_sharpness += [t.clone() for t in tail]
    assert not torch.isnan(log).any()
    want = {"iwe_variance": float(torch.stack(iwe_sharpness).mean())}
    for name, r in results.items():
        want[name] = r["metric"] / max(r["it"], 1)
    want_per = {f: {**{m: c["metric"] / c["it"] for m, c in d.items()}, "it": d["FWL"]["it"]} for f, d in per.items()}

    got = reduce_eval_log(log, tail, names, B, P, files)
    assert got.pop("per_sequence") == want_per and sorted(want_per) == ["a.npz", "b.npz", "c.npz"]
    assert want_per["a.npz"]["it"] == 4 and want_per["b.npz"]["it"] == 3 and want_per["c.npz"]["it"] == 3
    assert got == want
    assert set(reduce_eval_log(log, tail, names, B, P)) == {"iwe_variance", "FWL", "RSAT"}  # today's keys without the flag
    # no window at all: the eager loop's 0 / max(0, 1), the sharpness of the tail alone
    empty = reduce_eval_log(log[:0], tail, names, B, P)
    assert empty == {"iwe_variance": float(tail.mean()), "FWL": 0.0, "RSAT": 0.0}
    with pytest.raises(_lib.EvflowError, match="floats"):
        reduce_eval_log(log[:, :-1], tail, names, B, P)
    acc = PerSequence()
    acc.add("FWL", ["x", "x"], [1.0, 2.0])
    assert acc.summary() == {"x": {"FWL": 1.5, "it": 2}}
