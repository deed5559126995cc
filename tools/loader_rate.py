"""How fast do event windows reach the GPU from sequence files?  H5Loader (host slicing + one upload per batch) against
ResidentLoader (sequences uploaded once, windows cut by kernels), at the c3 data shape: B = 8 slots, passes of 1000 events,
128 x 128, P = 10 passes per window -> 80 samples per training step.

Cases, alternating inside one process after a warm-up, each timed for at least `--seconds` in all:
  h5_prefetch0      H5Loader, prefetch = 0 (host work in series with the launches)
  h5_prefetch2      H5Loader, prefetch = 2 (reader thread)
  resident_pass     ResidentLoader, per-pass iterator
  resident_window   ResidentLoader.next_window(10)
with and without the hot-pixel filter.  Reported: milliseconds per 80 samples, host clock around a final device
synchronise.  Sequence files: `.npz`, generated from --seed into a temporary directory (so no HDF5 reads are in the numbers).
The evaluation modes (time / gtflow windows, ResidentEvalLoader) are measured by tools/eval_loader_rate.py.

  python tools/loader_rate.py [--seconds 2] [--out profiles/loader_rate.json]
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

B, N, H, W, P, BINS = 8, 1000, 128, 128, 10, 2


def make_files(path, seed, files, events):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in range(files):
        ts = np.cumsum(rng.random(events) * 1e-5) + 10.0 * k
        write_npz_sequence(os.path.join(path, f"seq{k:02d}.npz"), rng.integers(0, W, events).astype(np.uint16),
                           rng.integers(0, H, events).astype(np.uint16), ts, rng.integers(0, 2, events).astype(np.uint8))


def config(path, hot):
    return {"data": {"path": path, "mode": "events", "window": N, "window_loss": P * N},
            "loader": {"batch_size": B, "resolution": [H, W], "augment": ["Horizontal", "Vertical", "Polarity"],
                       "augment_prob": [0.5, 0.5, 0.5]},
            "hot_filter": {"enabled": hot, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}, "vis": {"bars": False}}


class PerPass:
    """P batches of a loader's per-pass iterator per call; a new pass over the files when one ends."""

    def __init__(self, loader):
        self.loader, self.it = loader, None

    def window(self):
        got = 0
        while got < P:
            if self.it is None:
                self.it = iter(self.loader)
            batch = next(self.it, None)
            if batch is None:
                self.it = None
                continue
            got += 1
        return batch

    def close(self):
        if self.it is not None:
            self.it.close()


class PerWindow:
    def __init__(self, loader):
        self.loader = loader

    def window(self):
        return self.loader.next_window(P)

    def close(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--events", type=int, default=150000, help="events per sequence file")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"shape": {"B": B, "N": N, "H": H, "W": W, "P": P}, "unit": "ms per 80 samples", "files": args.files,
              "events_per_file": args.events}
    with tempfile.TemporaryDirectory() as tmp:
        make_files(tmp, args.seed, args.files, args.events)
        for hot in (False, True):
            np.random.seed(args.seed)
            cases = {"h5_prefetch0": PerPass(H5Loader(config(tmp, hot), BINS, prefetch=0)),
                     "h5_prefetch2": PerPass(H5Loader(config(tmp, hot), BINS, prefetch=2)),
                     "resident_pass": PerPass(ResidentLoader(config(tmp, hot), BINS)),
                     "resident_window": PerWindow(ResidentLoader(config(tmp, hot), BINS))}
            result.setdefault("resident_bytes", cases["resident_window"].loader.resident_bytes)
            for c in cases.values():  # warm-up: allocator, pinned blocks, first launches
                for _ in range(3):
                    c.window()
            torch.cuda.synchronize()
            spent = {k: 0.0 for k in cases}
            done = {k: 0 for k in cases}
            while min(spent.values()) < args.seconds:
                for name, c in cases.items():
                    if spent[name] >= args.seconds:
                        continue
                    t0 = time.perf_counter()
                    for _ in range(8):
                        c.window()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
                    done[name] += 8
            for c in cases.values():
                c.close()
            result["hot_filter_on" if hot else "hot_filter_off"] = {k: round(1e3 * spent[k] / done[k], 4) for k in cases}
            result["windows_timed_" + ("on" if hot else "off")] = done
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
