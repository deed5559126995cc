"""Streaming inference driver -- next to eval_flow.py: pushes ONE sequence file through `event_flow_amd.stream.FlowStream` in
chunks, as a camera or a socket would deliver it, and reports the windows run.  Every window of `data.window` events is one
table copy plus one hipGraph launch behind the warm-up; every chunk one pinned -> device copy plus one launch per appended slice.

  python infer_flow.py --config configs/eval_flow.yml --train-config configs/train_SNN.yml --sequence FILE [--weights model.pth]
                       [--chunk EVENTS]      # events per push (default: one window)
                       [--out DIR]           # flow_%06d.npy per window: the network's flow [2,H,W] (float32)
                       [--no-replay]         # the same launches without the graph replay

The configuration is eval_flow.py's (the eval YAML overlaid on the training YAML): data.window events per window, the sensor's
loader.resolution, hot_filter, the model.  `.npz` and HDF5 sequence files, as the loaders read them.  Prints one JSON line."""

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


def infer(args, config_parser):
    config = merged_config(args, config_parser)
    device = config_parser.device
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
    parser.add_argument("--sequence", required=True, metavar="FILE", help="one sequence file (.npz or HDF5)")
    parser.add_argument("--chunk", type=int, default=0, metavar="EVENTS", help="events per push (default: one window)")
    parser.add_argument("--out", default="", metavar="DIR", help="write flow_%%06d.npy per window")
    parser.add_argument("--no-replay", action="store_true", dest="no_replay", help="run every window's launches eagerly")
    args = parser.parse_args()
    infer(args, YAMLParser(args.config))
