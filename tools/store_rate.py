"""What does one STORED pass of eval_flow.py --store cost, and what does --render device change?  Both renderers of
utils/visualization.py on the same device tensors, through Visualization.store itself, at three shapes:
  events   B = 1, 180 x 240, data.mode events with the three window images: events, events_window, flow, flow_window, iwe, iwe_window
  gtflow   B = 1, 256 x 256 with a ground-truth map:                        events, flow, gtflow, iwe
  batched  B = 8, 128 x 128:                                                events, flow, iwe
           (the host renderer serves one slot at a time: measured as eight slot-wise store() calls per pass)
Quantities, in milliseconds per stored pass (host clock; every store() ends with the tensors on the host, the device one behind a
stream synchronise):
  host         render="host": up to eight device-to-host copies, numpy percentiles and HSV arithmetic
  device       render="device": one evf_render_sheet launch, one copy of the sheet into pinned memory
  *_png        the same with the PNG encoding (zlib) and the file writes; without the suffix write_png is replaced by a no-op
After a warm-up the four cases alternate, BLOCKS timed blocks of PASSES passes each; reported: the median over the blocks, and
the spread (min, max).  The inputs are seeded: Poisson counts with a mean of 0.3, an IWE with fractional values, normal flow.

  python tools/store_rate.py [--blocks 7] [--passes 8] [--out profiles/store_rate.json]
"""

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from event_flow_amd.utils import visualization as vis  # noqa: E402

DEV = "cuda:0"
SHAPES = {"events": dict(B=1, H=180, W=240, window=True, gtflow=False),
          "gtflow": dict(B=1, H=256, W=256, window=False, gtflow=True),
          "batched": dict(B=8, H=128, W=128, window=False, gtflow=False)}


def tensors(s, seed):
    r = np.random.default_rng(seed)
    B, H, W = s["B"], s["H"], s["W"]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)  # noqa: E731
    cnt, flow = f32(r.poisson(0.3, (B, 2, H, W))), f32(r.normal(0.0, 3.0, (B, 2, H, W)))
    iwe = f32(np.abs(r.normal(0.0, 0.6, (B, 2, H, W))))
    inputs = {"event_cnt": cnt}
    if s["gtflow"]:
        inputs["gtflow"] = f32(r.normal(0.0, 2.0, (B, 2, H, W)))
    win = (cnt * 3, flow * 0.5, iwe * 2.5) if s["window"] else (None, None, None)
    return inputs, flow, iwe, win


def store_pass(v, render, t, k):
    inputs, flow, iwe, win = t
    B = flow.shape[0]
    if render == "device":
        v.store(inputs, flow, iwe, ["slot%d" % b for b in range(B)], *win, ts=k)
        return
    for b in range(B):  # the host renderer: one slot per call
        one = lambda x: None if x is None else x[b:b + 1]  # noqa: E731
        v.store({n: one(x) for n, x in inputs.items()}, one(flow), one(iwe), "slot%d" % b, *[one(w) for w in win], ts=k)


def measure(name, s, blocks, passes, root):
    t = tensors(s, 7)
    real_png = vis.write_png
    cases = [(render, png) for render in ("host", "device") for png in (False, True)]
    stores = {c: vis.Visualization({}, eval_id=0, path_results=os.path.join(root, name, "%s_%d" % c) + "/", render=c[0]) for c in cases}
    times = {c: [] for c in cases}
    k = 0
    for block in range(blocks + 1):  # block 0: the warm-up (folders, code objects, the pinned buffer)
        for c in cases:
            vis.write_png = real_png if c[1] else (lambda path, img: None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                store_pass(stores[c], c[0], t, k)
                k += 1
            torch.cuda.synchronize()
            if block:
                times[c].append((time.perf_counter() - t0) * 1e3 / passes)
    vis.write_png = real_png
    out = {"B": s["B"], "H": s["H"], "W": s["W"], "images_per_slot": 3 + 3 * s["window"] + s["gtflow"]}
    for (render, png), v in times.items():
        out[render + ("_png" if png else "")] = {"ms_per_pass": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "store_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("store_rate.py measures on the GPU; no device found (nothing is reported from a CPU run)")
    torch.cuda.set_device(DEV)
    with tempfile.TemporaryDirectory() as root:
        res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "passes_per_block": a.passes,
               "unit": "milliseconds per stored pass, median over the timed blocks",
               "shapes": {name: measure(name, s, a.blocks, a.passes, root) for name, s in SHAPES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
