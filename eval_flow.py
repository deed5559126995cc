"""Evaluation driver -- counterpart of the reference's eval_flow.py:40-258 on the MI355X path: runs a model over
sequences, builds the per-polarity image of warped events (`compute_pol_iwe`) and accumulates FWL / RSAT / AEE
exactly as the reference loop does (association per input window, metric once `window_eval` events are collected).
No MLflow / visualiser; results are printed as JSON.

  python eval_flow.py --config configs/eval_flow.yml --train-config configs/train_SNN.yml --synthetic [--weights model.pth]
  python eval_flow.py ... --resident --graphed [--per-sequence]   # data.mode events: a graph launch per evaluated window;
                                                                  # gtflow_dt1 / gtflow_dt4 with metrics [AEE]: one per pass
  python eval_flow.py ... --store DIR [--render device]           # PNGs in the reference's folder layout; device: every image of
                                                                  # a pass and every slot of the batch from one evf_render_sheet launch
  python eval_flow.py ... --activity DIR                          # the reference's vis.activity: per pass the fraction of nonzero
                                                                  # outputs of the nine FireNet layers, counted on the device by one
                                                                  # launch per pass (every path above) -> DIR/activity.csv, "activity"
"""

import argparse
import json
import sys

import numpy as np
import torch

from event_flow_amd import _lib
from event_flow_amd import activity as activity_mod
from event_flow_amd.configs.parser import YAMLParser
from event_flow_amd.evaluate import PerSequence, ResidentAEEStep, ResidentEvalStep, graphed_refusal, slot_files
from event_flow_amd.loss import flow as metrics_mod
from event_flow_amd.models.model import MODELS
from event_flow_amd.utils.iwe import compute_pol_iwe
from event_flow_amd.utils.utils import load_model


def render_refusal(args, device):
    """Why --render does not serve these arguments (None: it does).  Host-only: asked before any device work."""
    render = getattr(args, "render", "host")
    if render == "host":
        return None
    if render != "device":
        return f"--render {render}: host or device"
    if not getattr(args, "store", ""):
        return "--render device colour-codes the STORED images on the GPU: add --store DIR, or drop --render device"
    if torch.device(device).type != "cuda":
        return (f"--render device runs evf_render_sheet on a CUDA device, and this evaluation runs on '{device}': use --render host "
                "(the numpy renderer)")
    return None


def store_folders(data, synthetic, B):
    """The folder of every batch slot for --store --render device: the stem of the file the slot reads now; the synthetic loader
    reads none and is numbered like the host renderer's folders.
    A slot that restarts takes sequence number max + 1 and opens files[number % len(files)], and the pass ends only after
    len(files) restarts, so with two or more slots a file can be opened a second time before the pass is over, even while
    another slot still reads it.  Every (slot, sequence number) is one visit with a folder of its own: the stem for a file's first
    visit (number < len(files)), `<stem>_visit<k>` for visit k = number // len(files) after it.  The numbers of the slots differ,
    so the names of a batch differ, never change while a slot stays on its sequence, and never come back.
    Asks the loader's slot table while the batch is out: the loader must not read ahead (H5Loader(prefetch=0))."""
    if synthetic:
        seq = getattr(data, "seq_num", 0)
        return ["seq%03d" % seq] if B == 1 else ["seq%03d_slot%d" % (seq, b) for b in range(B)]
    names = []
    for b, f in enumerate(slot_files(data)):
        visit = data.batch_idx[b] // len(data.files)
        names.append(f.split(".")[0] + ("_visit%d" % visit if visit else ""))
    return names


def test(args, config_parser, graphed_replay=True):
    """`graphed_replay=False`: with --graphed, the same launches without the graph replay (A/B, tests)."""
    # the reference overlays the eval YAML on the training run's stored parameters (merge_configs); here the
    # training YAML plays the role of the stored run
    train_cfg = YAMLParser(args.train_config).config
    config = config_parser.config
    merged = {k: (dict(v) if isinstance(v, dict) else v) for k, v in train_cfg.items()}
    for key, val in config.items():
        if isinstance(val, dict):
            merged.setdefault(key, {}).update(val)
        else:
            merged[key] = val
    config = config_parser.combine_entries(merged)
    config["data"].setdefault("window_eval", config["data"]["window"])
    config["loss"] = config.get("loss", {"overwrite_intermediate": False})
    device = config_parser.device
    graphed, per_sequence = getattr(args, "graphed", False), getattr(args, "per_sequence", False)
    model = None
    if graphed:  # refused on the host, before any device work (which path serves a network is a property of its cells)
        why = graphed_refusal(args, config)
        if not why:
            model = MODELS[config["model"]["name"]](config["model"].copy())
            why = graphed_refusal(args, config, model)
        if why:
            raise _lib.EvflowError(why)
    if per_sequence and args.synthetic:
        raise _lib.EvflowError("--per-sequence reports per sequence FILE; the synthetic loader reads none: drop --synthetic")
    why = render_refusal(args, device)
    if why:
        raise _lib.EvflowError(why)
    activity_dir = getattr(args, "activity", "") or ("." if config.get("vis", {}).get("activity", False) else "")
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(device)  # the evf_* launches go to the current device's stream (loader.gpu may not be 0)

    # configuration checks of the reference driver (eval_flow.py:54-73)
    names_cfg = config.get("metrics", {}).get("name", [])
    if "AEE" in names_cfg and not args.synthetic:  # (the synthetic loader carries one ground-truth map per input window)
        assert config["data"]["mode"] in ("gtflow_dt1", "gtflow_dt4"), "AEE computation not possible without ground truth mode"
        assert config["data"]["window"] <= 1, "AEE computation not compatible with window > 1"
        assert np.isclose((1.0 / config["data"]["window"]) % 1.0, 0.0), \
            "AEE computation not compatible with windows whose inverse is not a round number"
    if config["data"]["mode"] == "frames":
        if config["data"]["window"] <= 1.0:
            assert np.isclose((1.0 / config["data"]["window"]) % 1.0, 0.0), \
                "Frames mode not compatible with < 1 windows whose inverse is not a round number"
        else:
            assert np.isclose(config["data"]["window"] % 1.0, 0.0), "Frames mode not compatible with > 1 fractional windows"

    model = (model if model is not None else MODELS[config["model"]["name"]](config["model"].copy())).to(device)
    if args.weights:  # a state_dict file, a reference checkpoint (pickled model) or its MLflow run id under ./mlruns
        model = load_model(args.weights, model, device)
    model.eval()
    activity_path = None
    if activity_dir:  # asked on the host: the device log (fused FireNets), model(..., log=True) (general-path FireNets) or refused
        activity_path = activity_mod.path(model)
        if activity_path is None:
            raise _lib.EvflowError(activity_mod.refusal(model))
        if activity_path == "host":
            print(activity_mod.refusal(model), file=sys.stderr)

    names = config.get("metrics", {}).get("name", [])
    criteria = [getattr(metrics_mod, m)(config, device, flow_scaling=config["metrics"]["flow_scaling"]) for m in names]

    if args.synthetic:
        from event_flow_amd.dataloader.synthetic_loader import SyntheticLoader

        data = SyntheticLoader(config, config["model"]["num_bins"], device=device, num_sequences=args.sequences)
    elif getattr(args, "resident", False):  # the sequence files uploaded once, every batch cut and filtered on the GPU
        if config["data"]["mode"] == "events":
            from event_flow_amd.dataloader.resident import ResidentLoader as Resident
        else:  # windows by time, frame or ground-truth map: borders searched once, ragged batches, resident maps / frames
            from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader as Resident

        data = Resident(config, config["model"]["num_bins"], device=device)
    else:
        from event_flow_amd.dataloader.h5 import H5Loader

        # (--per-sequence and --render device ask the loader which file a slot reads while its batch is out: no reader thread
        # running ahead, which advances batch_idx before the batches of the old sequence have been consumed)
        ask_slots = per_sequence or (bool(args.store) and getattr(args, "render", "host") == "device")
        data = H5Loader(config, config["model"]["num_bins"], device=device, **({"prefetch": 0} if ask_slots else {}))

    vis = None
    render = getattr(args, "render", "host")
    if args.store:  # stored PNGs in the reference's folder layout (utils/visualization.py:120-226); --render host: batch size 1
        from event_flow_amd.utils.visualization import Visualization

        vis = Visualization(config, eval_id=0, path_results=args.store.rstrip("/") + "/", render=render)
    # the three window images (reference eval_flow.py:201-210): events mode, input windows shorter than the evaluated one
    window_images = vis is not None and config["data"]["mode"] == "events" and config["data"]["window"] < config["data"]["window_eval"]
    if graphed and config["data"]["mode"] != "events":  # (graphed_refusal: AEE alone on ground-truth windows)
        return _test_graphed_aee(config, model, data, per_sequence, graphed_replay, activity_dir)
    if graphed:
        return _test_graphed(config, model, criteria, names, data, per_sequence, graphed_replay, activity_dir)
    per_seq = PerSequence() if per_sequence else None
    B = config["loader"]["batch_size"]
    act_log = activity_mod.ActivityLog(model, B) if activity_path == "device" else None
    act_report = activity_mod.Report(activity_dir, B, per_sequence) if activity_path else None
    act_new, act_files, act_host = [], ([] if per_sequence else None), []

    def drain_activity():
        if act_log is not None:
            batch, slots = act_log.fractions(act_log.drain())
        else:  # the nine reads of every pass were made by model(..., log=True)
            batch, slots = np.array(act_host, dtype=np.float64).reshape(-1, len(activity_mod.LAYERS)), None
        act_report.add(batch, slots, act_new, act_files)
        del act_new[:], act_host[:]
        if act_files is not None:
            del act_files[:]

    results = {m: {"metric": 0.0, "it": 0, **({"percent": 0.0} if m == "AEE" else {})} for m in names}
    iwe_sharpness = []
    idx_AEE = 0  # sub-windows since the last AEE evaluation (eval_flow.py:117,171-176)
    aee_every = 1 if args.synthetic else int(np.round(1.0 / config["data"]["window"]))
    with torch.no_grad():
        for inputs in data:
            restarted = bool(data.new_seq)
            if data.new_seq:
                data.new_seq = False
                model.reset_states()
            if getattr(data, "pass_done", False):  # every sequence was visited (eval_flow.py:124-127)
                break
            if activity_path == "host":
                x = model(inputs["event_voxel"], inputs["event_cnt"], log=True)
                act_host.append([x["activity"][layer] for layer in activity_mod.LAYERS])
            else:
                x = model(inputs["event_voxel"], inputs["event_cnt"])
            if activity_path:
                if act_log is not None:
                    if act_log.full:
                        drain_activity()
                    act_log.record(*model.last_io())
                act_new.append(restarted)
                if act_files is not None:
                    act_files.append(slot_files(data))
            iwe = compute_pol_iwe(x["flow"][-1], inputs["event_list"], config["loader"]["resolution"],
                                  inputs["event_list_pol_mask"][:, :, 0:1], inputs["event_list_pol_mask"][:, :, 1:2],
                                  flow_scaling=config["metrics"]["flow_scaling"], round_idx=True)
            iwe_sharpness.append(iwe.sum(1).var(dim=(1, 2)).mean())
            storing = vis is not None and (render == "device" or iwe.shape[0] == 1)
            if storing:
                flow_vis = x["flow"][-1] * inputs["event_mask"] if config["model"].get("mask_output", True) else x["flow"][-1]
            window_vis = (None, None, None)
            for metric in criteria:
                metric.event_flow_association(x["flow"], inputs)
            for i, name in enumerate(names):
                if criteria[i].num_events >= config["data"]["window_eval"]:
                    if config["loss"].get("overwrite_intermediate", False):
                        criteria[i].overwrite_intermediate_flow(x["flow"])
                    if name == "AEE":
                        # no ground truth interval yet: skip WITHOUT resetting; with window < 1 the ground-truth map
                        # spans round(1/window) input windows, so the criterion keeps accumulating until the last
                        # of them and is evaluated (and reset) only then (eval_flow.py:169-176)
                        if float(torch.as_tensor(inputs["dt_gt"]).reshape(-1)[0]) <= 0.0:
                            continue
                        idx_AEE += 1
                        if idx_AEE != aee_every:
                            continue
                    val = criteria[i]()
                    if name == "AEE":
                        idx_AEE = 0
                    results[name]["it"] += 1
                    if name == "AEE":
                        results[name]["metric"] += float(val[0].mean())
                        results[name]["percent"] += float(val[1].mean())
                    else:
                        results[name]["metric"] += float(val.mean())
                    if per_seq is not None:  # a slot's value goes to the file that slot reads now (eval_flow.py:183-199)
                        files = slot_files(data)
                        if name == "AEE":
                            per_seq.add("AEE", files, val[0].reshape(-1).tolist())
                            per_seq.add("AEE_percent_outliers", files, val[1].reshape(-1).tolist())
                        else:
                            per_seq.add(name, files, val.reshape(-1).tolist())
                    if i == 0 and storing and window_images:  # the first metric's window, before its reset
                        window_vis = (criteria[i].compute_window_events(), criteria[i].compute_masked_window_flow(),
                                      criteria[i].compute_window_iwe())
                    criteria[i].reset()
            if storing:  # (after the metrics, as in the reference: eval_flow.py:221-232)
                sequence = store_folders(data, args.synthetic, iwe.shape[0]) if render == "device" else "seq%03d" % getattr(data, "seq_num", 0)
                vis.store(inputs, flow_vis, iwe, sequence, *window_vis, ts=getattr(data, "last_proc_timestamp", None))
    out = {"model": config["model"]["name"], "iwe_variance": float(torch.stack(iwe_sharpness).mean())}
    for name, r in results.items():
        out[name] = r["metric"] / max(r["it"], 1)
        if name == "AEE":
            out["AEE_percent_outliers"] = r["percent"] / max(r["it"], 1)
    if per_seq is not None:
        out["per_sequence"] = per_seq.summary()
    if activity_path:
        drain_activity()
        act_report.into(out)
        if act_log is not None:
            act_log.close()
    print(json.dumps(out))
    return out


def _stepper_activity(model, B, passes, directory, per_sequence):
    """The activity log of a replayed evaluation, sized for its passes (the host knows them: no ring), and its report."""
    if not directory:
        return None, None
    return (activity_mod.ActivityLog(model, B, rows=max(passes, 1)), activity_mod.Report(directory, B, per_sequence))


def _test_graphed(config, model, criteria, names, data, per_sequence, replay, activity_dir=""):
    """The loop above for `data.mode: events` on the resident loader, an evaluated window (P = ceil(window_eval / window)
    batches) per step: one table copy and one graph launch each, the results read once at the end (evaluate.py)."""
    P = -(-int(config["data"]["window_eval"]) // int(config["data"]["window"]))
    steps = list(data.plan_eval_steps(P))  # host-only: the number of evaluated windows sizes the result log
    act_log, report = _stepper_activity(model, data.batch_size, sum(len(group) for group, _r, _t in steps), activity_dir, per_sequence)
    stepper = ResidentEvalStep(model, criteria, names, data, P, len(steps) - 1, config["metrics"]["flow_scaling"],
                               overwrite_intermediate=config["loss"].get("overwrite_intermediate", False), replay=replay,
                               per_sequence=per_sequence, activity=act_log)
    stepper.activity_report = report
    model.reset_states()
    for group, pass_reset, tail in steps:
        if tail:
            stepper.step_tail(group, pass_reset)
        else:
            stepper.step(group, pass_reset)
    out = {"model": config["model"]["name"], **stepper.results(), "graphed": dict(stepper.stats)}
    print(json.dumps(out))
    return out


def _test_graphed_aee(config, model, data, per_sequence, replay, activity_dir=""):
    """The loop above for AEE alone in `data.mode` gtflow_dt1 / gtflow_dt4 on the resident loader, a PASS per step: one table
    copy and one graph launch each; which passes evaluate (the `idx_AEE` rule), how many there are and the width of the
    replayed buffers come from the host-only plan, the results are read once at the end (evaluate.ResidentAEEStep)."""
    plan = list(data.plan_eval_passes())
    capacity = max([job[2] for jobs, _restarted, _evaluate in plan for job in jobs] + [1])
    evaluations = sum(1 for _jobs, _restarted, evaluate in plan if evaluate)
    act_log, report = _stepper_activity(model, data.batch_size, len(plan), activity_dir, per_sequence)
    stepper = ResidentAEEStep(model, data, len(plan), evaluations, capacity, config["metrics"]["flow_scaling"], replay=replay,
                              per_sequence=per_sequence, activity=act_log)
    stepper.activity_report = report
    model.reset_states()
    for jobs, restarted, evaluate in plan:
        stepper.step(jobs, restarted, evaluate)
    out = {"model": config["model"]["name"], **stepper.results(),
           "graphed": {**stepper.stats, "passes": stepper.seen, "evaluations": stepper.evaluated, "capacity": capacity}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="configs/eval_flow.yml")
    parser.add_argument("--train-config", default="configs/train_SNN.yml", help="configuration the model was trained with")
    parser.add_argument("--weights", default="", help="state_dict (reference: the run id)")
    parser.add_argument("--synthetic", action="store_true")
    parser.add_argument("--sequences", type=int, default=4)
    parser.add_argument("--resident", action="store_true",
                        help="keep the sequence files in device memory and cut the input windows there (every data.mode: "
                             "ResidentLoader for events, ResidentEvalLoader with resident ground-truth maps / frames for time, "
                             "frames, gtflow_dt1 and gtflow_dt4)")
    parser.add_argument("--graphed", action="store_true",
                        help="with --resident and data.mode events: every evaluated window (window_eval events) is one job-table "
                             "copy plus one hipGraph launch, results logged on the device and read once at the end (fused "
                             "LIF / PLIF / XLIF / ALIF FireNets; FWL / RSAT); with data.mode gtflow_dt1 / gtflow_dt4 and metrics.name "
                             "[AEE]: every PASS is one job-table copy plus one hipGraph launch, AEE reduced on the device")
    parser.add_argument("--per-sequence", action="store_true", dest="per_sequence",
                        help="also report every metric per sequence file (\"per_sequence\": {file: {metric: mean, \"it\": n}})")
    parser.add_argument("--activity", default="", metavar="DIR",
                        help="the reference's vis.activity (vis.activity: True in the configuration means --activity .): per pass "
                             "the fraction of nonzero outputs of the nine FireNet layers, counted exactly on the device by one launch "
                             "per pass -- inside the replayed graphs of --graphed as well -- and read once -> DIR/activity.csv and "
                             "\"activity\" in the JSON (with --per-sequence per file, too); a general-path FireNet falls back to "
                             "model(..., log=True) on the host")
    parser.add_argument("--store", default="", help="directory that receives results/eval_0/<sequence>/{events,flow,iwe,...}/*.png; "
                                                    "in data.mode events with window < window_eval also events_window, flow_window and "
                                                    "iwe_window, at every pass whose first metric fired")
    parser.add_argument("--render", choices=["host", "device"], default="host",
                        help="with --store: host colour-codes every image in numpy (batch size 1, one sequence slot); device "
                             "colour-codes every image of a pass and every slot of the batch in one evf_render_sheet launch and one "
                             "copy, slot b under the stem of the file it reads (needs --store and a CUDA device)")
    args = parser.parse_args()
    test(args, YAMLParser(args.config))
