"""How long does one pass of the AEE evaluation take, and what does the AEE itself cost?  LIFFireNet, metrics [AEE],
data.mode gtflow_dt1 with window 1, flow_scaling 128, hot-pixel filter on, synthetic sequences of about 20 000 events per
ground-truth map, at two shapes:
  mvsec    the reference's configs/eval_MVSEC.yml: B = 1 slot, 256 x 256
  batched  B = 8 slots, 256 x 256

Part 1, cases alternating inside one process after a warm-up, each timed for at least `--seconds` in all:
  h5_eager          eval_flow.py: the loop on H5Loader (reader thread, host formatting, one eager forward per pass)
  resident_eager    eval_flow.py --resident: the same loop on ResidentEvalLoader
  resident_graphed  eval_flow.py --resident --graphed: ResidentAEEStep, one table copy + one graph launch per pass
The eager loops read dt_gt and the metric on the host as the driver does; the graphed one reads its logs once at the end.
Reported: milliseconds per pass (every pass forwards and, with a map behind every window, evaluates), host clock around a
final device synchronise.

Part 2, the AEE alone on static inputs of the same shape, both forms captured REP times into one graph and replayed:
  aee_old  the float32 division of the two ratios, evf_aee (one block per sample) and the torch tail of AEE.forward and of the
           log row: two divisions, a sum, two means, evf_store_segments_at
  aee_at   evf_aee_at (two launches)
Reported: microseconds per AEE (HIP events around the replays, divided by REP).

  python tools/eval_aee_rate.py [--seconds 2] [--out profiles/eval_aee_rate.json]
"""

import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from event_flow_amd import _lib  # noqa: E402
from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence  # noqa: E402
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader  # noqa: E402
from event_flow_amd.evaluate import ResidentAEEStep  # noqa: E402
from event_flow_amd.loss.flow import AEE  # noqa: E402
from event_flow_amd.models.model import LIFFireNet  # noqa: E402
from event_flow_amd.utils.iwe import compute_pol_iwe  # noqa: E402

DEV = "cuda:0"
BINS, SCALING, REP = 2, 128, 16
SHAPES = {"mvsec": dict(B=1, H=256, W=256, files=2, maps=30, events_per_map=20000),
          "batched": dict(B=8, H=256, W=256, files=8, maps=30, events_per_map=20000)}
MODEL_CFG = {"num_bins": BINS, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
             "activations": ["arctanspike", "arctanspike"],
             "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}


def make_files(path, seed, s):
    rng = np.random.Generator(np.random.PCG64(seed))
    H, W = s["H"], s["W"]
    for k in range(s["files"]):
        n = s["maps"] * s["events_per_map"]
        ts = 10.0 * (k + 1) + np.sort(rng.random(n)) * 0.05 * s["maps"]
        stamps = 10.0 * (k + 1) + 0.05 * np.arange(s["maps"] + 1)
        maps = [(f"{m:06d}", stamps[m], rng.standard_normal((2, H, W)).astype(np.float32)) for m in range(s["maps"] + 1)]
        write_npz_sequence(os.path.join(path, f"seq{k:02d}.npz"), rng.integers(0, W, n).astype(np.uint16),
                           rng.integers(0, H, n).astype(np.uint16), ts, rng.integers(0, 2, n).astype(np.uint8), flow_dt1=maps)


def config(path, s):
    return {"data": {"path": path, "mode": "gtflow_dt1", "window": 1, "window_eval": 1},
            "loader": {"batch_size": s["B"], "resolution": [s["H"], s["W"]], "augment": [], "augment_prob": []},
            "loss": {"overwrite_intermediate": False}, "metrics": {"name": ["AEE"], "flow_scaling": SCALING},
            "hot_filter": {"enabled": True, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}, "vis": {"bars": False}}


def network(thresh_scale):
    torch.manual_seed(0)
    model = LIFFireNet(dict(MODEL_CFG)).to(DEV)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("thresh"):
                p.mul_(thresh_scale)
    model.eval()
    return model


class EagerLoop:
    """eval_flow.py's loop on `iter(loader)`, one forwarded pass per step; pass after pass over the files."""

    def __init__(self, loader_cls, cfg, thresh_scale):
        self.cfg = cfg
        self.model, self.metric = network(thresh_scale), AEE(cfg, DEV, flow_scaling=SCALING)
        self.data = loader_cls(cfg, BINS, device=DEV)
        self.it = None
        self.sharp, self.total, self.percent, self.evaluated = [], 0.0, 0.0, 0

    def step(self):
        cfg = self.cfg
        with torch.no_grad():
            while True:
                if self.it is None:
                    self.it = iter(self.data)
                inputs = next(self.it, None)
                if inputs is None:
                    self.it = None
                    continue
                if self.data.new_seq:
                    self.data.new_seq = False
                    self.model.reset_states()
                if getattr(self.data, "pass_done", False):
                    self.it.close()
                    self.it = None
                    continue
                x = self.model(inputs["event_voxel"], inputs["event_cnt"])
                iwe = compute_pol_iwe(x["flow"][-1], inputs["event_list"], cfg["loader"]["resolution"],
                                      inputs["event_list_pol_mask"][:, :, 0:1], inputs["event_list_pol_mask"][:, :, 1:2],
                                      flow_scaling=SCALING, round_idx=True)
                self.sharp = [iwe.sum(1).var(dim=(1, 2)).mean()]
                self.metric.event_flow_association(x["flow"], inputs)
                if float(torch.as_tensor(inputs["dt_gt"]).reshape(-1)[0]) > 0.0:  # (window 1: every counted pass evaluates)
                    val = self.metric()
                    self.total += float(val[0].mean())
                    self.percent += float(val[1].mean())
                    self.evaluated += 1
                    self.metric.reset()
                return


class GraphedLoop:
    def __init__(self, cfg, thresh_scale, rows=1 << 18):
        self.data = ResidentEvalLoader(cfg, BINS, device=DEV)
        first = list(self.data.plan_eval_passes())  # (host-only: the widest window of a pass over the files)
        capacity = max([job[2] for jobs, _r, _e in first for job in jobs] + [1])
        self.stepper = ResidentAEEStep(network(thresh_scale), self.data, rows, rows, capacity, SCALING)
        self.plan = None

    def step(self):
        while True:
            if self.plan is None:
                self.plan = self.data.plan_eval_passes()
            nxt = next(self.plan, None)
            if nxt is None:
                self.plan = None
                continue
            self.stepper.step(*nxt)
            return


def aee_alone(s, seed, replays=200):
    """Part 2 -> microseconds per AEE of the two forms."""
    B, H, W = s["B"], s["H"], s["W"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    flow = torch.randn((B, 2, H, W), generator=g, device=DEV) * 0.01
    gt = torch.randn((B, 2, H, W), generator=g, device=DEV)
    mask = (torch.rand((B, H, W), generator=g, device=DEV) < 0.3).float()
    dt_gt = torch.full((B,), 0.05, dtype=torch.float64, device=DEV)
    dt_input = torch.full((B,), 0.049, dtype=torch.float64, device=DEV)
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    log = torch.zeros((4, 2 * (B + 1)), dtype=torch.float32, device=DEV)
    ws = torch.empty(B * _lib.load().evf_aee_at_stripes(H, W) * 3, dtype=torch.float32, device=DEV)

    def old():
        ratio = (torch.as_tensor(dt_gt, dtype=torch.float32) / torch.as_tensor(dt_input, dtype=torch.float32)).contiguous()
        out = torch.empty((B, 3), dtype=torch.float32, device=DEV)
        _lib.call("evf_aee", _lib.ptr(flow), _lib.ptr(gt), _lib.ptr(mask), _lib.ptr(ratio), B, H, W, float(SCALING), _lib.ptr(out))
        aee = (out[:, 0] / (out[:, 1] + 1e-9)).contiguous()
        pct = (out[:, 2].sum() / (out[:, 1] + 1e-9)).contiguous()
        src = [aee, aee.mean().view(1), pct, pct.mean().view(1)]
        _lib.call("evf_store_segments_at", _lib.ptr(row), 4, _lib.ptr(log), 2 * (B + 1), (ctypes.c_void_p * 32)(*[_lib.ptr(t) for t in src]),
                  (ctypes.c_int * 32)(0, B, B + 1, 2 * B + 1), (ctypes.c_int * 32)(B, 1, B, 1), 4)
        return src

    def new():
        _lib.call("evf_aee_at", _lib.ptr(flow), _lib.ptr(gt), _lib.ptr(mask), _lib.ptr(dt_gt), _lib.ptr(dt_input), B, H, W, float(SCALING),
                  _lib.ptr(row), 4, _lib.ptr(log), 2 * (B + 1), 0, _lib.ptr(ws), ws.numel())

    us = {}
    stream = torch.cuda.Stream()
    for name, fn in (("aee_old", old), ("aee_at", new)):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            keep = [fn() for _ in range(REP)]
        for _ in range(20):
            graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us[name] = round(1e3 * e0.elapsed_time(e1) / (replays * REP), 3)
        del keep
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (0.25: an alive network)")
    ap.add_argument("--shapes", default="mvsec,batched")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"model": "LIFFireNet", "metrics": ["AEE"], "mode": "gtflow_dt1", "unit": "ms per pass; us per AEE", "hot_filter": True,
              "thresh_scale": args.thresh_scale, "device": torch.cuda.get_device_name(0), "aee_per_graph": REP}
    for shape in args.shapes.split(","):
        s = SHAPES[shape]
        with tempfile.TemporaryDirectory() as tmp:
            make_files(tmp, args.seed, s)
            cfg = config(tmp, s)
            np.random.seed(args.seed)
            cases = {"h5_eager": EagerLoop(H5Loader, cfg, args.thresh_scale),
                     "resident_eager": EagerLoop(ResidentEvalLoader, cfg, args.thresh_scale),
                     "resident_graphed": GraphedLoop(cfg, args.thresh_scale)}
            for c in cases.values():  # warm-up: allocator, pinned blocks, first launches, the two graphs
                for _ in range(6):
                    c.step()
            torch.cuda.synchronize()
            spent = {k: 0.0 for k in cases}
            done = {k: 0 for k in cases}
            while min(spent.values()) < args.seconds:
                for name, c in cases.items():
                    if spent[name] >= args.seconds:
                        continue
                    t0 = time.perf_counter()
                    for _ in range(8):
                        c.step()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
                    done[name] += 8
            stepper = cases["resident_graphed"].stepper
            result[shape] = {"shape": {k: s[k] for k in ("B", "H", "W")}, "files": s["files"], "maps_per_file": s["maps"],
                             "events_per_map": s["events_per_map"], "capacity": stepper.window.capacity,
                             "ms_per_pass": {k: round(1e3 * spent[k] / done[k], 4) for k in cases}, "passes_timed": done,
                             "counters": {**stepper.stats, "evaluations": stepper.evaluated},
                             "us_per_aee": aee_alone(s, args.seed)}
            for c in cases.values():  # (H5Loader's reader thread ends with its iterator)
                it = getattr(c, "it", None)
                if it is not None:
                    it.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
