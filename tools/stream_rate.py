"""How long does one window of streaming inference take?  LIFFireNet on count input, at two shapes:
  ecd    1 x 180 x 240, windows of 15000 events (the reference's configs/eval_ECD.yml)
  mvsec  1 x 256 x 256, windows of 20000 events

Cases, alternating inside one process after a warm-up, each timed for at least `--seconds` in all; every case is fed the same
host arrays one window at a time and restarts its sequence when the file ends:
  hand_eager       what a user writes today: the window formatted on the host (event_formatting's float32 normalisation), one
                   host -> device copy, encode_event_list, model(...); no hot-pixel filter (the host one is the loader's)
  stream_eager     FlowStream(replay=False).push: one chunk copy + evf_ring_append, then the window's launches, hot filter on
  stream           FlowStream.push: the same with the window's launches as one graph launch
  resident_eager   the yardstick: eval_flow.py --resident without metrics -- the loop on ResidentLoader (the file uploaded once),
                   one eager forward per batch, hot filter on
Reported: milliseconds per window, host clock around a final device synchronise; `push_until_ready_ms`: the host time of one
push of a whole window until its `ready` event has passed (median and mean of --latency pushes, the stream otherwise idle);
`launch_us`: the mean duration of the stream's own three launches in the eager stream (HIP events around each call).

  python tools/stream_rate.py [--seconds 2] [--out profiles/stream_rate.json]
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

from event_flow_amd import _lib  # noqa: E402
from event_flow_amd.dataloader.encodings import encode_event_list  # noqa: E402
from event_flow_amd.dataloader.h5 import write_npz_sequence  # noqa: E402
from event_flow_amd.dataloader.resident import ResidentLoader  # noqa: E402
from event_flow_amd.models.model import LIFFireNet  # noqa: E402
from event_flow_amd.stream import FlowStream  # noqa: E402

DEV = "cuda:0"
BINS = 2
SHAPES = {"ecd": dict(H=180, W=240, N=15000, windows=60), "mvsec": dict(H=256, W=256, N=20000, windows=60)}
MODEL_CFG = {"num_bins": BINS, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
             "activations": ["arctanspike", "arctanspike"],
             "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}


def make_events(seed, s):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = s["N"] * s["windows"]
    return (rng.integers(0, s["W"], n).astype(np.uint16), rng.integers(0, s["H"], n).astype(np.uint16),
            np.cumsum(rng.random(n) * 1e-5) + 10.0, rng.integers(0, 2, n).astype(np.uint8))


def config(path, s):
    return {"data": {"path": path, "mode": "events", "window": s["N"]},
            "loader": {"batch_size": 1, "resolution": [s["H"], s["W"]], "augment": [], "augment_prob": []},
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


class Windows:
    """The file's windows, one after the other, again and again."""

    def __init__(self, cols, s):
        self.cols, self.N, self.n, self.k = cols, s["N"], s["windows"], 0

    def next(self):
        k, self.k = self.k, (self.k + 1) % self.n
        return k == 0, [c[k * self.N:(k + 1) * self.N] for c in self.cols]


class HandEager(Windows):
    def __init__(self, cols, s, thresh_scale):
        super().__init__(cols, s)
        self.res, self.model = (s["H"], s["W"]), model(thresh_scale)

    def step(self):
        new, (xs, ys, ts, ps) = self.next()
        if new:
            self.model.reset_states()
        t = ts.astype(np.float32)
        rows = np.stack([(t - t[0]) / (t[-1] - t[0]), ys.astype(np.float32), xs.astype(np.float32), ps.astype(np.float32) * 2 - 1], 1)
        with torch.no_grad():
            d = encode_event_list(torch.from_numpy(rows[None]).to(DEV), BINS, self.res, want=("cnt", "mask"))
            self.flow = self.model(None, d["event_cnt"])["flow"][-1]


class Streamed(Windows):
    def __init__(self, cols, s, cfg, thresh_scale, replay):
        super().__init__(cols, s)
        self.stream = FlowStream(model(thresh_scale), cfg, window=s["N"], t0=float(cols[2][0]), replay=replay)

    def step(self):
        new, cols = self.next()
        if new and self.stream.appended:
            self.stream.reset()
        (self.last,) = self.stream.push(*cols)


class ResidentEager:
    def __init__(self, cfg, thresh_scale):
        self.model, self.data, self.it = model(thresh_scale), ResidentLoader(cfg, BINS, device=DEV), None

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
                return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (0.25: an alive network)")
    ap.add_argument("--latency", type=int, default=200, help="pushes timed one by one until `ready`")
    ap.add_argument("--shapes", default="ecd,mvsec")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"model": "LIFFireNet", "unit": "ms per window", "hot_filter": {"hand_eager": False, "others": True},
              "thresh_scale": args.thresh_scale, "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        s = SHAPES[shape]
        cols = make_events(args.seed, s)
        with tempfile.TemporaryDirectory() as tmp:
            write_npz_sequence(os.path.join(tmp, "seq00.npz"), *cols)
            cfg = config(tmp, s)
            np.random.seed(args.seed)
            cases = {"hand_eager": HandEager(cols, s, args.thresh_scale),
                     "stream_eager": Streamed(cols, s, cfg, args.thresh_scale, False),
                     "stream": Streamed(cols, s, cfg, args.thresh_scale, True),
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
                    t0 = time.perf_counter()
                    for _ in range(8):
                        c.step()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
                    done[name] += 8
            out = {"shape": {k: s[k] for k in ("H", "W", "N")}, "windows_in_file": s["windows"],
                   "ms": {k: round(1e3 * spent[k] / done[k], 4) for k in cases}, "windows_timed": done,
                   "counters": dict(cases["stream"].stream.stats)}
            # one push of a window until its result is ready, the stream otherwise idle
            out["push_until_ready_ms"] = {}
            for name in ("stream_eager", "stream"):
                lat = []
                for _ in range(args.latency):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cases[name].step()
                    cases[name].last.ready.synchronize()
                    lat.append(1e3 * (time.perf_counter() - t0))
                out["push_until_ready_ms"][name] = {"median": round(float(np.median(lat)), 4), "mean": round(float(np.mean(lat)), 4)}
            # the stream's own launches, eager, bracketed by HIP events
            names = ["evf_ring_append", "evf_ring_cut", "evf_store_segments_at"]
            _lib.profile_start(names)
            for _ in range(50):
                cases["stream_eager"].step()
            prof = _lib.profile_stop()
            out["launch_us"] = {n: round(1e3 * float(np.mean([v for (k, _var), vs in prof.items() if k == n for v in vs])), 2) for n in names}
            result[shape] = out
            it = cases["resident_eager"].it
            if it is not None:
                it.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
