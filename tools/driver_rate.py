"""How long does one optimizer step of the training driver take on device-resident sequences?  c3 shape: LIFFireNet, B = 8 slots,
128 x 128, passes of 1000 events, P = 10 passes per step, FlatAdam.

Cases, alternating inside one process after a warm-up, each timed for at least `--seconds` in all:
  pass_loop       train_flow.py --resident: one eager forward per pass, the loss's backward and the optimizer per step
  window_eager    ResidentWindowStep(replay=False): one cut per window, the window's launches eagerly (train_window)
  window_replay   ResidentWindowStep: one job-table copy + one graph launch per step (train_flow.py --resident --graphed)
with and without the hot-pixel filter.  Reported: milliseconds per optimizer step, host clock around a final device
synchronise.  Sequence files: `.npz`, generated from --seed into a temporary directory.

  python tools/driver_rate.py [--seconds 2] [--out profiles/driver_rate.json]
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

from loader_rate import B, BINS, H, N, P, W, config, make_files  # noqa: E402

from event_flow_amd.dataloader.resident import ResidentLoader  # noqa: E402
from event_flow_amd.loss.flow import EventWarping  # noqa: E402
from event_flow_amd.models.model import LIFFireNet  # noqa: E402
from event_flow_amd.train import FlatAdam, ResidentWindowStep  # noqa: E402

DEV = "cuda:0"
MODEL_CFG = {"num_bins": BINS, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
             "activations": ["arctanspike", "arctanspike"],
             "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}
LOSS_CFG = {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False, "clip_grad": 100.0},
            "model": {"mask_output": True}}


def parts(path, hot, thresh_scale, device_step):
    torch.manual_seed(0)
    model = LIFFireNet(dict(MODEL_CFG)).to(DEV)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("thresh"):
                p.mul_(thresh_scale)
    model.train()
    opt = FlatAdam(model, lr=2e-4, clip=100.0, device_step=device_step)
    opt.zero_grad()
    return model, EventWarping(LOSS_CFG, DEV), opt, ResidentLoader(config(path, hot), BINS)


class PassLoop:
    """train_flow.py's loop on `iter(loader)`, until one optimizer step is taken."""

    def __init__(self, path, hot, thresh_scale):
        self.model, self.lossf, self.opt, self.data = parts(path, hot, thresh_scale, False)
        self.it = None

    def step(self):
        while True:
            if self.it is None:
                self.it = iter(self.data)
            inputs = next(self.it, None)
            if inputs is None:
                self.it = None
                continue
            if self.data.new_seq:
                self.data.new_seq = False
                self.lossf.reset()
                self.model.reset_states()
                self.opt.zero_grad()
            x = self.model(inputs["event_voxel"], inputs["event_cnt"])
            self.lossf.event_flow_association(x["flow"], inputs["event_list"], inputs["event_list_pol_mask"], inputs["event_mask"])
            if self.lossf.num_events >= P * N:
                loss = self.lossf()
                loss.backward()
                self.opt.step()
                self.opt.zero_grad()
                self.model.detach_states()
                self.lossf.reset()
                return loss.detach()


class WindowLoop:
    def __init__(self, path, hot, thresh_scale, replay):
        model, lossf, opt, data = parts(path, hot, thresh_scale, True)
        self.stepper = ResidentWindowStep(model, lossf, opt, data, P, replay=replay)

    def step(self):
        return self.stepper.step()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--events", type=int, default=150000, help="events per sequence file")
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (bench.py's switch; 0.25: an alive network)")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"shape": {"B": B, "N": N, "H": H, "W": W, "P": P}, "model": "LIFFireNet", "unit": "ms per optimizer step",
              "files": args.files, "events_per_file": args.events, "thresh_scale": args.thresh_scale,
              "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        make_files(tmp, args.seed, args.files, args.events)
        for hot in (False, True):
            np.random.seed(args.seed)
            cases = {"pass_loop": PassLoop(tmp, hot, args.thresh_scale),
                     "window_eager": WindowLoop(tmp, hot, args.thresh_scale, False),
                     "window_replay": WindowLoop(tmp, hot, args.thresh_scale, True)}
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
            key = "hot_filter_on" if hot else "hot_filter_off"
            result[key] = {k: round(1e3 * spent[k] / done[k], 4) for k in cases}
            result["steps_timed_" + ("on" if hot else "off")] = done
            result["counters_" + ("on" if hot else "off")] = dict(cases["window_replay"].stepper.stats)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
