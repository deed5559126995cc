"""How fast do EVALUATION batches reach the GPU from sequence files?  H5Loader (per batch: host searches, host slicing, a host
flip of the ground-truth map, uploads) against ResidentEvalLoader (sequences, maps and window borders resident; batches cut and
gathered by kernels), at two shapes on 256 x 256 sequences:

  gtflow_dt1_B1   data.mode gtflow_dt1, window 1, one slot -- the shape of the reference's MVSEC evaluation config
  time_B8         data.mode time, windows of --time-window seconds, eight slots

Cases per shape, alternating inside one process after a warm-up, each timed for at least `--seconds` in all:
  h5_prefetch0    H5Loader, prefetch = 0 (host work in series with the launches)
  h5_prefetch2    H5Loader, prefetch = 2 (reader thread)
  resident        ResidentEvalLoader
Reported: milliseconds per batch (host clock around a final device synchronise), and per shape the seconds the constructor of
each loader took (for the resident one: reading and uploading every file, and the one search).  Sequence files: `.npz`,
generated from --seed into a temporary directory (no HDF5 reads in the numbers); no augmentation, no hot-pixel filter.

  python tools/eval_loader_rate.py [--seconds 2] [--out profiles/eval_loader_rate.json]
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
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader  # noqa: E402

H = W = 256
BINS = 2
DT = 0.05  # seconds between two ground-truth maps


def make_files(path, seed, files, maps, events_per_map):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = maps * events_per_map
    for k in range(files):
        t0 = 100.0 * (k + 1)
        ts = t0 + np.sort(rng.random(n)) * (maps * DT)
        stamps = t0 + DT * np.arange(maps + 1)
        stamps[0] = ts[0]
        gt = [(f"{i:06d}", stamps[i], rng.standard_normal((2, H, W)).astype(np.float32)) for i in range(maps + 1)]
        write_npz_sequence(os.path.join(path, f"seq{k:02d}.npz"), rng.integers(0, W, n).astype(np.uint16),
                           rng.integers(0, H, n).astype(np.uint16), ts, rng.integers(0, 2, n).astype(np.uint8), flow_dt1=gt)


def config(path, mode, window, B):
    return {"data": {"path": path, "mode": mode, "window": window},
            "loader": {"batch_size": B, "resolution": [H, W], "augment": [], "augment_prob": []},
            "hot_filter": {"enabled": False, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}, "vis": {"bars": False}}


class Batches:
    """One batch of a loader's iterator per call; a new pass over the files when one ends."""

    def __init__(self, make):
        t0 = time.perf_counter()
        self.loader = make()
        torch.cuda.synchronize()
        self.built = time.perf_counter() - t0
        self.it = None

    def batch(self):
        while True:
            if self.it is None:
                self.it = iter(self.loader)
            batch = next(self.it, None)
            if batch is not None:
                return batch
            self.it = None

    def close(self):
        if self.it is not None:
            self.it.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--maps", type=int, default=30, help="ground-truth intervals per sequence file")
    ap.add_argument("--events-per-map", type=int, default=20000)
    ap.add_argument("--time-window", type=float, default=0.01)
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_loader_rate.py measures on the GPU only")
    result = {"unit": "ms per batch", "resolution": [H, W], "files": args.files, "maps_per_file": args.maps + 1,
              "events_per_file": args.maps * args.events_per_map}
    shapes = {"gtflow_dt1_B1": ("gtflow_dt1", 1, 1), "time_B8": ("time", args.time_window, 8)}
    with tempfile.TemporaryDirectory() as tmp:
        make_files(tmp, args.seed, args.files, args.maps, args.events_per_map)
        for shape, (mode, window, B) in shapes.items():
            cfg = config(tmp, mode, window, B)
            cases = {"h5_prefetch0": Batches(lambda: H5Loader(cfg, BINS, prefetch=0)),
                     "h5_prefetch2": Batches(lambda: H5Loader(cfg, BINS, prefetch=2)),
                     "resident": Batches(lambda: ResidentEvalLoader(cfg, BINS))}
            for c in cases.values():  # warm-up: allocator, pinned blocks, first launches
                for _ in range(8):
                    c.batch()
            torch.cuda.synchronize()
            spent = {k: 0.0 for k in cases}
            done = {k: 0 for k in cases}
            while min(spent.values()) < args.seconds:
                for name, c in cases.items():
                    if spent[name] >= args.seconds:
                        continue
                    t0 = time.perf_counter()
                    for _ in range(16):
                        c.batch()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
                    done[name] += 16
            for c in cases.values():
                c.close()
            result[shape] = {"mode": mode, "window": window, "B": B,
                             "ms_per_batch": {k: round(1e3 * spent[k] / done[k], 4) for k in cases},
                             "batches_timed": done,
                             "construction_s": {k: round(c.built, 4) for k, c in cases.items()},
                             "resident_bytes": cases["resident"].loader.resident_bytes}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
