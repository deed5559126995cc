"""Streaming inference driver -- next to eval_flow.py: pushes ONE sequence file through `event_flow_amd.stream.FlowStream` in
chunks, as a camera or a socket would deliver it, and reports the windows run.  Every window of `data.window` events is one
table copy plus one hipGraph launch behind the warm-up; every chunk one pinned -> device copy plus one launch per appended slice.
With --window-dt the windows are cut by TIME instead, through `event_flow_amd.rig_stream.RigStream`: one --sequence per camera of a
synchronised rig (one file: the single-camera time-window stream), the rows of all files pushed in time order.

  python infer_flow.py --config configs/eval_flow.yml --train-config configs/train_SNN.yml --sequence FILE [--weights model.pth]
                       [--chunk EVENTS]      # events per push (default: one window)
                       [--out DIR]           # flow_%06d.npy per window: the network's flow [2,H,W] (float32)
                       [--no-replay]         # the same launches without the graph replay
                       [--window-dt SECONDS] # windows of SECONDS by time (flow at a fixed rate); --sequence once per camera
                       [--max-events N]      # ... of at most N events per camera (default: data.window when it is a count, else 30000)

The configuration is eval_flow.py's (the eval YAML overlaid on the training YAML): data.window events per window, the sensor's
loader.resolution, hot_filter, the model.  `.npz` and HDF5 sequence files, as the loaders read them.  Prints one JSON line.
With --window-dt, --out holds flow_%06d.npy of shape [cameras,2,H,W], and --chunk counts the events of all cameras together."""

import argparse
import json
import os
import time

import numpy as np
import torch

from event_flow_amd import _lib
from event_flow_amd.configs.parser import YAMLParser
from event_flow_amd.dataloader.h5 import open_sequence
from event_flow_amd.dataloader.resident_base import read_columns
from event_flow_amd.models.model import MODELS
from event_flow_amd.rig_stream import RigStream
from event_flow_amd.stream import FlowStream, stream_refusal
from event_flow_amd.utils.utils import load_model


def merged_config(args, config_parser):
    """eval_flow.py's overlay of the eval YAML on the training run's parameters."""
    train_cfg = YAMLParser(args.train_config).config
    merged = {k: (dict(v) if isinstance(v, dict) else v) for k, v in train_cfg.items()}
    for key, val in config_parser.config.items():
        if isinstance(val, dict):
            merged.setdefault(key, {}).update(val)
        else:
            merged[key] = val
    return config_parser.combine_entries(merged)


def infer_rig(args, config, device):
    """--window-dt: the files of `args.sequence`, one per camera, through a `RigStream` in time order.  A push holds the next
    --chunk rows of the merged files; in front of it the watermark is declared up to its first timestamp (in time order every
    camera has delivered everything before it), in steps that complete fewer windows than the result ring has rows."""
    dt = float(args.window_dt)
    window = config["data"]["window"]
    count_window = not isinstance(window, bool) and window >= 2 and int(window) == window
    max_events = int(args.max_events) if args.max_events else (int(window) if count_window else 30000)
    chunk = int(args.chunk) if args.chunk else max_events
    if not dt > 0 or max_events < 1 or chunk < 1:
        raise _lib.EvflowError(f"--window-dt {args.window_dt} --max-events {max_events} --chunk {chunk}: all three are positive")
    model = MODELS[config["model"]["name"]](config["model"].copy())
    why = stream_refusal(model)  # on the host, before any device work
    if why:
        raise _lib.EvflowError(why)
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(device)
    model = model.to(device)
    if args.weights:
        model = load_model(args.weights, model, device)
    model.eval()

    cams, t0 = [], None
    for name in args.sequence:
        seq = open_sequence(name)
        xs, ys, _rel, ps, ts = read_columns(seq, name)
        t0 = float(seq.attrs["t0"]) if t0 is None else min(t0, float(seq.attrs["t0"]))
        seq.close()
        cams.append((xs, ys, ts, ps))
    B, slots = len(cams), 8
    rig = RigStream(model, config, cameras=B, window_dt=dt, max_events=max_events, capacity=2 * max_events + chunk, slots=slots, t0=t0,
                    replay=not args.no_replay, device=device)
    # the rows of all files in time order (a stable sort: equal timestamps in camera order)
    cam_of = np.concatenate([np.full(len(c[2]), b, dtype=np.int64) for b, c in enumerate(cams)])
    order = np.argsort(np.concatenate([c[2] for c in cams]), kind="stable")
    cam_of, when = cam_of[order], np.concatenate([c[2] for c in cams])[order]
    step = (slots - 2) * dt  # (a span that crosses at most `slots` - 1 borders)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    torch.cuda.synchronize()
    windows = 0

    def took(results):
        nonlocal windows
        for r in results:
            if args.out:
                r.ready.synchronize()
                np.save(os.path.join(args.out, "flow_%06d.npy" % r.index), r.flow.cpu().numpy())
            windows += 1

    def declare(t):
        while rig.plan.declared < t:
            took(rig.advance(min(t, max(rig.plan.declared, t0) + step)))

    begin = time.perf_counter()
    at, lo = [0] * B, 0
    while lo < len(when):
        declare(float(when[lo]))
        hi = min(lo + chunk, len(when), int(np.searchsorted(when, when[lo] + step, side="left")))
        hi = max(hi, lo + 1)
        take = np.bincount(cam_of[lo:hi], minlength=B)
        took(rig.push([tuple(c[a:a + n] for c in cam) for cam, a, n in zip(cams, at, take)]))
        at, lo = [a + int(n) for a, n in zip(at, take)], hi
    if len(when):
        declare(float(when[-1]))
    rig.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - begin) * 1e3
    out = {"model": config["model"]["name"], "sequences": [os.path.basename(s) for s in args.sequence], "cameras": B,
           "events": [int(len(c[0])) for c in cams], "window_dt": dt, "max_events": max_events, "chunk": chunk, "windows": windows,
           "pending": rig.plan.uncut, "stream": dict(rig.stats), "ms_per_window": ms / max(windows, 1)}
    print(json.dumps(out))
    return out


def infer(args, config_parser):
    config = merged_config(args, config_parser)
    device = config_parser.device
    if getattr(args, "window_dt", None):
        return infer_rig(args, config, device)
    if isinstance(args.sequence, (list, tuple)):
        if len(args.sequence) != 1:
            raise _lib.EvflowError(f"{len(args.sequence)} --sequence files: windows by event count serve one camera; a rig needs "
                                   "--window-dt SECONDS (time windows line up across cameras)")
        args.sequence = args.sequence[0]
    window = config["data"]["window"]
    if isinstance(window, bool) or int(window) != window or window < 2:
        raise _lib.EvflowError(f"infer_flow.py cuts windows of data.window EVENTS (an integer >= 2), got {window!r}: windows by time "
                               "are served by eval_flow.py --resident")
    window = int(window)
    chunk = int(args.chunk) if args.chunk else window
    if chunk < 1:
        raise _lib.EvflowError(f"--chunk {args.chunk}: at least one event per push")
    model = MODELS[config["model"]["name"]](config["model"].copy())
    why = stream_refusal(model)  # on the host, before any device work
    if why:
        raise _lib.EvflowError(why)
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(device)
    model = model.to(device)
    if args.weights:
        model = load_model(args.weights, model, device)
    model.eval()

    seq = open_sequence(args.sequence)
    xs, ys, _rel, ps, ts = read_columns(seq, args.sequence)  # (the absolute timestamps: the stream subtracts t0 as read_columns does)
    t0 = float(seq.attrs["t0"])
    seq.close()
    stream = FlowStream(model, config, window=window, t0=t0, replay=not args.no_replay, device=device)
    chunk = min(chunk, stream.slots * window - window + 1)  # (the longest push that is accepted whatever is pending)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    torch.cuda.synchronize()
    windows = 0
    begin = time.perf_counter()
    for lo in range(0, len(xs), chunk):
        for r in stream.push(xs[lo:lo + chunk], ys[lo:lo + chunk], ts[lo:lo + chunk], ps[lo:lo + chunk]):
            if args.out:
                r.ready.synchronize()
                np.save(os.path.join(args.out, "flow_%06d.npy" % r.index), r.flow.cpu().numpy())
            windows += 1
    stream.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - begin) * 1e3
    out = {"model": config["model"]["name"], "sequence": os.path.basename(args.sequence), "events": int(len(xs)), "window": window,
           "chunk": chunk, "windows": windows, "pending": int(stream.pending), "stream": dict(stream.stats),
           "ms_per_window": ms / max(windows, 1)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="configs/eval_flow.yml")
    parser.add_argument("--train-config", default="configs/train_SNN.yml", help="configuration the model was trained with")
    parser.add_argument("--weights", default="", help="state_dict (reference: the run id)")
    parser.add_argument("--sequence", required=True, action="append", metavar="FILE",
                        help="one sequence file (.npz or HDF5); with --window-dt repeatable, one file per camera")
    parser.add_argument("--chunk", type=int, default=0, metavar="EVENTS", help="events per push (default: one window)")
    parser.add_argument("--out", default="", metavar="DIR", help="write flow_%%06d.npy per window")
    parser.add_argument("--window-dt", type=float, default=0.0, dest="window_dt", metavar="SECONDS",
                        help="cut windows of SECONDS by time (RigStream) instead of data.window events")
    parser.add_argument("--max-events", type=int, default=0, dest="max_events", metavar="N",
                        help="with --window-dt: events per camera and window at most (a fuller window is refused)")
    parser.add_argument("--no-replay", action="store_true", dest="no_replay", help="run every window's launches eagerly")
    args = parser.parse_args()
    infer(args, YAMLParser(args.config))
