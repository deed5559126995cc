"""How long does one tick of a rig stream take -- one window of `dt` seconds for B synchronised cameras?  LIFFireNet on count
input, windows of dt = 10 ms, B = 1, 2, 4 and 8, at two shapes:
  ecd    B x 180 x 240, about 15000 events per camera and window (`max_events` 16000)
  mvsec  B x 256 x 256, about 20000 events per camera and window (`max_events` 21000)

Cases, alternating inside one process after a warm-up, each timed for at least `--seconds` in all; every case reads the same
recordings (one per camera, different events) and starts them again when they end:
  rig              RigStream.push of one window's events of every camera: one staged copy + evf_rings_append, then the tick the
                   push completes as one table copy and one graph launch; hot filter on
  rig_eager        RigStream(replay=False): the same with the tick's launches made one by one
  resident_eager   the yardstick, what the project could do before: eval_flow.py --resident in `data.mode: time` without metrics
                   -- the loop on ResidentEvalLoader (the files uploaded once, batch size B), one eager forward per batch; hot filter on
  b1_times_B       B times the `rig` figure of B = 1: B single-camera streams one after the other (computed, not run)
Reported: milliseconds per tick (per batch for the loader), host clock around a final device synchronise; `per_camera`: the same
divided by B.

  python tools/rig_stream_rate.py [--seconds 1.5] [--out profiles/rig_stream_rate.json]
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

from event_flow_amd.dataloader.h5 import write_npz_sequence  # noqa: E402
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader  # noqa: E402
from event_flow_amd.models.model import LIFFireNet  # noqa: E402
from event_flow_amd.rig_stream import RigStream  # noqa: E402

DEV = "cuda:0"
BINS = 2
DT = 0.01
T0 = 10.0
SHAPES = {"ecd": dict(H=180, W=240, N=15000, max_events=16000, windows=40),
          "mvsec": dict(H=256, W=256, N=20000, max_events=21000, windows=40)}
MODEL_CFG = {"num_bins": BINS, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
             "activations": ["arctanspike", "arctanspike"],
             "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}


def make_camera(seed, s):
    """One camera's recording: `windows` windows of 0.9 N .. N events with distinct ascending timestamps, the first exactly T0,
    and one event behind the last border (it completes the last window) -> (xs, ys, ts, ps)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ts, row = [], 0.0
    for _k in range(s["windows"]):
        n = int(rng.integers(int(0.9 * s["N"]), s["N"] + 1))
        ts.append(row + T0 + (np.arange(n) + 0.25 + 0.5 * rng.random(n)) / n * DT * 0.96)
        row += DT
    ts = np.concatenate(ts + [[row + T0 + 0.3 * DT]])
    ts[0] = T0
    n = len(ts)
    return rng.integers(0, s["W"], n).astype(np.uint16), rng.integers(0, s["H"], n).astype(np.uint16), ts, rng.integers(0, 2, n).astype(np.uint8)


def config(path, s, B):
    return {"data": {"path": path, "mode": "time", "window": DT},
            "loader": {"batch_size": B, "resolution": [s["H"], s["W"]], "augment": [], "augment_prob": []},
            "hot_filter": {"enabled": True, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}, "vis": {"bars": False}}


def model(thresh_scale):
    torch.manual_seed(0)
    m = LIFFireNet(dict(MODEL_CFG)).to(DEV)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("thresh"):
                p.mul_(thresh_scale)
    m.eval()
    return m


class Rig:
    """The recordings pushed one window of every camera at a time, again and again; a step ends with one completed tick."""

    def __init__(self, cams, s, cfg, thresh_scale, replay):
        self.cams, self.n, self.k = cams, s["windows"], 0
        # (where every window starts in every camera; the last slice holds the event behind the last border too)
        self.cuts = [np.searchsorted(c[2], T0 + DT * np.arange(self.n + 1)) for c in cams]
        for cut, c in zip(self.cuts, cams):
            cut[-1] = len(c[2])
        self.stream = RigStream(model(thresh_scale), cfg, cameras=len(cams), window_dt=DT, max_events=s["max_events"], t0=T0,
                                replay=replay)
        self.ticks = 0

    def push(self):
        k, self.k = self.k, (self.k + 1) % self.n
        if k == 0 and self.ticks:
            self.stream.reset()
        out = self.stream.push([tuple(col[cut[k]:cut[k + 1]] for col in c) for c, cut in zip(self.cams, self.cuts)])
        self.ticks += len(out)
        return out

    def step(self):
        while not self.push():
            pass


class ResidentEager:
    def __init__(self, cfg, thresh_scale):
        self.model, self.data, self.it = model(thresh_scale), ResidentEvalLoader(cfg, BINS, device=DEV), None
        self.ticks = 0

    def step(self):
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
                self.flow = self.model(inputs["event_voxel"], inputs["event_cnt"])["flow"][-1]
                self.ticks += 1
                return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (0.25: an alive network)")
    ap.add_argument("--shapes", default="ecd,mvsec")
    ap.add_argument("--cameras", default="1,2,4,8")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"model": "LIFFireNet", "unit": "ms per tick (one window of every camera)", "window_dt": DT, "hot_filter": True,
              "thresh_scale": args.thresh_scale, "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        s = SHAPES[shape]
        out = {"shape": {k: s[k] for k in ("H", "W", "N", "max_events")}, "windows_in_file": s["windows"], "cameras": {}}
        for B in (int(b) for b in args.cameras.split(",")):
            cams = [make_camera(args.seed + 100 * b, s) for b in range(B)]
            with tempfile.TemporaryDirectory() as tmp:
                for b, c in enumerate(cams):
                    write_npz_sequence(os.path.join(tmp, "seq%02d.npz" % b), *c)
                cfg = config(tmp, s, B)
                np.random.seed(args.seed)
                cases = {"rig": Rig(cams, s, cfg, args.thresh_scale, True), "rig_eager": Rig(cams, s, cfg, args.thresh_scale, False),
                         "resident_eager": ResidentEager(cfg, args.thresh_scale)}
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
                        t0, before = time.perf_counter(), c.ticks
                        for _ in range(8):
                            c.step()
                        torch.cuda.synchronize()
                        spent[name] += time.perf_counter() - t0
                        done[name] += c.ticks - before  # (the push that ends a recording completes two ticks)
                ms = {k: round(1e3 * spent[k] / done[k], 4) for k in cases}
                out["cameras"][str(B)] = {"ms": ms, "ticks_timed": done, "counters": dict(cases["rig"].stream.stats)}
                it = cases["resident_eager"].it
                if it is not None:
                    it.close()
                del cases
        if "1" in out["cameras"]:
            one = out["cameras"]["1"]["ms"]["rig"]
            for B, o in out["cameras"].items():
                o["ms"]["b1_times_B"] = round(one * int(B), 4)
        for B, o in out["cameras"].items():
            o["per_camera"] = {k: round(v / int(B), 4) for k, v in o["ms"].items()}
        result[shape] = out
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
