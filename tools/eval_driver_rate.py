"""How long does one evaluated window of the evaluation driver take?  LIFFireNet, FWL + RSAT, flow_scaling 128, hot-pixel filter
on, at two shapes:
  ecd      the reference's configs/eval_ECD.yml: B = 1 slot, 180 x 240, window = window_eval = 15000 events (P = 1 pass)
  batched  B = 8 slots, 128 x 128, passes of 1000 events, window_eval 10000 (P = 10 passes)

Cases, alternating inside one process after a warm-up, each timed for at least `--seconds` in all:
  h5_eager          eval_flow.py: the loop on H5Loader (reader thread, host formatting, one eager forward per pass)
  resident_eager    eval_flow.py --resident: the same loop on ResidentLoader
  resident_graphed  eval_flow.py --resident --graphed: ResidentEvalStep, one table copy + one graph launch per window
The eager loops read every metric on the host when it fires (`float(val.mean())`), as the driver does; the graphed one reads
its log once at the end.  Reported: milliseconds per evaluated window, host clock around a final device synchronise.  The
graphed case skips the tail of a pass over the files (fewer than P batches, never evaluated).  Sequence files: `.npz`,
generated from --seed into a temporary directory.

  python tools/eval_driver_rate.py [--seconds 2] [--out profiles/eval_driver_rate.json]
"""

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from event_flow_amd.dataloader.h5 import H5Loader, write_npz_sequence  # noqa: E402
from event_flow_amd.dataloader.resident import ResidentLoader  # noqa: E402
from event_flow_amd.evaluate import ResidentEvalStep  # noqa: E402
from event_flow_amd.loss.flow import FWL, RSAT  # noqa: E402
from event_flow_amd.models.model import LIFFireNet  # noqa: E402
from event_flow_amd.utils.iwe import compute_pol_iwe  # noqa: E402

DEV = "cuda:0"
BINS, SCALING = 2, 128
SHAPES = {"ecd": dict(B=1, H=180, W=240, N=15000, P=1, files=3, events=1500000),
          "batched": dict(B=8, H=128, W=128, N=1000, P=10, files=12, events=150000)}
MODEL_CFG = {"num_bins": BINS, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
             "activations": ["arctanspike", "arctanspike"],
             "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}


def make_files(path, seed, s):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in range(s["files"]):
        n = s["events"]
        ts = np.cumsum(rng.random(n) * 1e-5) + 10.0 * k
        write_npz_sequence(os.path.join(path, f"seq{k:02d}.npz"), rng.integers(0, s["W"], n).astype(np.uint16),
                           rng.integers(0, s["H"], n).astype(np.uint16), ts, rng.integers(0, 2, n).astype(np.uint8))


def config(path, s):
    return {"data": {"path": path, "mode": "events", "window": s["N"], "window_eval": s["P"] * s["N"]},
            "loader": {"batch_size": s["B"], "resolution": [s["H"], s["W"]], "augment": [], "augment_prob": []},
            "loss": {"overwrite_intermediate": False}, "metrics": {"name": ["FWL", "RSAT"], "flow_scaling": SCALING},
            "hot_filter": {"enabled": True, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}, "vis": {"bars": False}}


def parts(cfg, thresh_scale):
    torch.manual_seed(0)
    model = LIFFireNet(dict(MODEL_CFG)).to(DEV)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("thresh"):
                p.mul_(thresh_scale)
    model.eval()
    return model, [FWL(cfg, DEV, flow_scaling=SCALING), RSAT(cfg, DEV, flow_scaling=SCALING)]


class EagerLoop:
    """eval_flow.py's loop on `iter(loader)`, until the metrics have fired once; pass after pass over the files."""

    def __init__(self, loader_cls, cfg, thresh_scale):
        self.cfg = cfg
        self.model, self.criteria = parts(cfg, thresh_scale)
        self.data = loader_cls(cfg, BINS, device=DEV)
        self.it = None
        self.sharp, self.total = [], 0.0

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
                fired = False
                for metric in self.criteria:
                    metric.event_flow_association(x["flow"], inputs)
                for metric in self.criteria:
                    if metric.num_events >= cfg["data"]["window_eval"]:
                        self.total += float(metric().mean())
                        metric.reset()
                        fired = True
                if fired:
                    return


class GraphedLoop:
    def __init__(self, cfg, thresh_scale, P, rows=1 << 16):
        model, criteria = parts(cfg, thresh_scale)
        self.data = ResidentLoader(cfg, BINS, device=DEV)
        self.P = P
        self.stepper = ResidentEvalStep(model, criteria, ["FWL", "RSAT"], self.data, P, rows, SCALING)
        self.plan = None

    def step(self):
        while True:
            if self.plan is None:
                self.plan = self.data.plan_eval_steps(self.P)
            group, pass_reset, tail = next(self.plan)
            if tail:
                self.plan.close()
                self.plan = None
                continue
            self.stepper.step(group, pass_reset)
            return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (0.25: an alive network)")
    ap.add_argument("--shapes", default="ecd,batched")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"model": "LIFFireNet", "metrics": ["FWL", "RSAT"], "unit": "ms per evaluated window", "hot_filter": True,
              "thresh_scale": args.thresh_scale, "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        s = SHAPES[shape]
        with tempfile.TemporaryDirectory() as tmp:
            make_files(tmp, args.seed, s)
            cfg = config(tmp, s)
            np.random.seed(args.seed)
            cases = {"h5_eager": EagerLoop(H5Loader, cfg, args.thresh_scale),
                     "resident_eager": EagerLoop(ResidentLoader, cfg, args.thresh_scale),
                     "resident_graphed": GraphedLoop(cfg, args.thresh_scale, s["P"])}
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
            result[shape] = {"shape": {k: s[k] for k in ("B", "H", "W", "N", "P")}, "files": s["files"], "events_per_file": s["events"],
                             "ms": {k: round(1e3 * spent[k] / done[k], 4) for k in cases}, "windows_timed": done,
                             "counters": dict(cases["resident_graphed"].stepper.stats)}
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
