"""What does the activity log (activity.ActivityLog, evf_activity_at) cost per pass?  LIFFireNet at the two evaluation shapes of
tools/eval_driver_rate.py and tools/eval_aee_rate.py, with their files, configurations and loops:
  ecd    B = 1, 180 x 240, 15000 events a pass, FWL / RSAT in data.mode events (ResidentEvalStep, P = 1)
  mvsec  B = 1, 256 x 256, about 20 000 events a ground-truth map, AEE in gtflow_dt1 (ResidentAEEStep)

(a) replayed: the stepper with the log attached against the same stepper without it (`activity=None`: not one launch, buffer or
    table word differs from the graph before the log existed), alternating inside one process after a warm-up, each timed for at
    least `--seconds`: milliseconds per replayed step, host clock around a final device synchronise.
(b) eager: model(x) + ActivityLog.record against model(x, log=True) (the flush, nine .item() reads and the [B,32,H,W] float
    expansion of every spike tensor) and against model(x) alone, on a static input of the shape: milliseconds per pass.
(c) the kernel alone, captured REP times into one graph and replayed, on static sources of the shape, for several splits of a
    source into parts (ACT_CHUNK elements a block, at most ACT_MAX_PARTS parts; built from csrc/evf_activity.hip alone into
    tools/_ab/): microseconds per call (HIP events around the replays, divided by REP).  This is what decided the split.

  python tools/eval_activity_rate.py [--seconds 2] [--out profiles/eval_activity_rate.json]
"""

import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import eval_aee_rate as aee_rate  # noqa: E402
import eval_driver_rate as drv_rate  # noqa: E402
from event_flow_amd import _lib, build  # noqa: E402
from event_flow_amd.activity import KINDS, LAYERS, ActivityLog  # noqa: E402
from event_flow_amd.dataloader.resident import ResidentLoader  # noqa: E402
from event_flow_amd.dataloader.resident_eval import ResidentEvalLoader  # noqa: E402
from event_flow_amd.evaluate import ResidentAEEStep, ResidentEvalStep  # noqa: E402

DEV = "cuda:0"
REP, ROWS = 16, 1 << 14
SPLITS = [(1 << 27, 1), (65536, 64), (32768, 64), (16384, 64), (8192, 64), (4096, 64), (2048, 256), (1024, 256)]  # (ACT_CHUNK, ACT_MAX_PARTS)


class WindowLoop(drv_rate.GraphedLoop):
    def __init__(self, cfg, thresh_scale, P, logged):
        model, criteria = drv_rate.parts(cfg, thresh_scale)
        self.data = ResidentLoader(cfg, drv_rate.BINS, device=DEV)
        self.P = P
        self.log = ActivityLog(model, self.data.batch_size, rows=ROWS * P) if logged else None
        self.stepper = ResidentEvalStep(model, criteria, ["FWL", "RSAT"], self.data, P, ROWS, drv_rate.SCALING, activity=self.log)
        self.plan = None


class PassLoop(aee_rate.GraphedLoop):
    def __init__(self, cfg, thresh_scale, logged):
        self.data = ResidentEvalLoader(cfg, aee_rate.BINS, device=DEV)
        first = list(self.data.plan_eval_passes())
        capacity = max([job[2] for jobs, _r, _e in first for job in jobs] + [1])
        model = aee_rate.network(thresh_scale)
        self.log = ActivityLog(model, self.data.batch_size, rows=ROWS) if logged else None
        self.stepper = ResidentAEEStep(model, self.data, ROWS, ROWS, capacity, aee_rate.SCALING, activity=self.log)
        self.plan = None


def alternate(cases, seconds, chunk=8):
    """ms per step of every case, the cases taking turns (`chunk` steps and a device synchronise a turn)."""
    for c in cases.values():  # warm-up: allocator, pinned blocks, first launches, the two graphs
        for _ in range(6):
            c.step()
    torch.cuda.synchronize()
    spent, done = {k: 0.0 for k in cases}, {k: 0 for k in cases}
    while min(spent.values()) < seconds:
        for name, c in cases.items():
            if spent[name] >= seconds:
                continue
            t0 = time.perf_counter()
            for _ in range(chunk):
                c.step()
            torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            done[name] += chunk
    return {k: round(1e3 * spent[k] / done[k], 4) for k in cases}, done


class EagerPass:
    def __init__(self, s, thresh_scale, how, seed):
        self.model = aee_rate.network(thresh_scale)
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.x = torch.poisson(torch.full((s["B"], 2, s["H"], s["W"]), 0.2, device=DEV), generator=g)
        self.how = how
        self.log = ActivityLog(self.model, s["B"], rows=1024) if how == "record" else None

    def step(self):
        with torch.no_grad():
            if self.how == "log_true":
                self.model(None, self.x, log=True)
            else:
                self.model(None, self.x)
                if self.log is not None:
                    if self.log.full:
                        self.log.drain()
                    self.log.record(*self.model.last_io())


def variant(chunk, max_parts):
    """csrc/evf_activity.hip alone as a shared library with another split (tools/_ab/, built when absent)."""
    out = os.path.join(ROOT, "tools", "_ab", f"libact_{chunk}_{max_parts}.so")
    src = os.path.join(build.CSRC, "evf_activity.hip")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build.HIPCC] + build.FLAGS + [f"-DACT_CHUNK={chunk}", f"-DACT_MAX_PARTS={max_parts}", "-shared", src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.evf_activity_parts.argtypes = _lib.SIGNATURES["evf_activity_parts"]
    lib.evf_activity_at.argtypes = _lib.SIGNATURES["evf_activity_at"]
    return lib


def kernel_alone(s, seed, replays=200):
    """(c) -> {split: {"parts", "us"}} and the library's own split."""
    B, H, W = s["B"], s["H"], s["W"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.poisson(torch.full((B, 2, H, W), 0.2, device=DEV), generator=g)
    words = [torch.randint(-2 ** 31, 2 ** 31 - 1, (B, H, W), generator=g, device=DEV, dtype=torch.int64).to(torch.int32) for _ in range(7)]
    flow = torch.randn((B, 2, H, W), generator=g, device=DEV)
    src = [x] + words + [flow]
    n = [2 * H * W] + [H * W] * 7 + [2 * H * W]
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    srcs = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in src])
    kinds, ns = (ctypes.c_int * 9)(*KINDS), (ctypes.c_int64 * 9)(*n)
    stream = torch.cuda.Stream()
    out, first = {}, None
    libs = [("library", _lib.load())] + [(f"{c}/{m}", variant(c, m)) for c, m in SPLITS]
    for name, lib in libs:
        parts = int(lib.evf_activity_parts(max(n)))
        log = torch.zeros((4, 9, B, parts), dtype=torch.int32, device=DEV)

        def call():
            rc = lib.evf_activity_at(srcs, kinds, ns, 9, B, row.data_ptr(), 1, 0, 4, log.data_ptr(), torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                raise RuntimeError(f"evf_activity_at ({name}) failed with status {rc}")

        call()
        torch.cuda.synchronize()
        counts = log[0].cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=2)
        first = counts if first is None else first
        if not np.array_equal(counts, first):
            raise RuntimeError(f"split {name} counts differently")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(REP):
                call()
        for _ in range(20):
            graph.replay()
        best = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            best.append(1e3 * e0.elapsed_time(e1) / (replays * REP))
        out[name] = {"parts": parts, "us": round(min(best), 3), "us_runs": [round(v, 3) for v in best]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per case, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresh-scale", type=float, default=1.0, help="multiply every firing threshold (0.25: an alive network)")
    ap.add_argument("--shapes", default="ecd,mvsec")
    ap.add_argument("--out", default="", help="also write the result line to this file")
    args = ap.parse_args()
    result = {"model": "LIFFireNet", "layers": list(LAYERS), "unit": "ms per replayed step / eager pass; us per evf_activity_at",
              "thresh_scale": args.thresh_scale, "device": torch.cuda.get_device_name(0), "calls_per_graph": REP,
              "train_monitor_percent": 2.2}
    for shape in args.shapes.split(","):
        with tempfile.TemporaryDirectory() as tmp:
            np.random.seed(args.seed)
            if shape == "ecd":
                s = drv_rate.SHAPES["ecd"]
                drv_rate.make_files(tmp, args.seed, s)
                cfg = drv_rate.config(tmp, s)
                cases = {"graphed": WindowLoop(cfg, args.thresh_scale, s["P"], False), "graphed_activity": WindowLoop(cfg, args.thresh_scale, s["P"], True)}
            else:
                s = aee_rate.SHAPES["mvsec"]
                aee_rate.make_files(tmp, args.seed, s)
                cfg = aee_rate.config(tmp, s)
                cases = {"graphed": PassLoop(cfg, args.thresh_scale, False), "graphed_activity": PassLoop(cfg, args.thresh_scale, True)}
            ms, done = alternate(cases, args.seconds)
            eager = {how: EagerPass(s, args.thresh_scale, how, args.seed) for how in ("forward", "record", "log_true")}
            ems, edone = alternate(eager, args.seconds / 2)
            result[shape] = {"shape": {k: s[k] for k in ("B", "H", "W")},
                             "replayed_ms_per_step": ms, "replayed_steps_timed": done, "counters": dict(cases["graphed_activity"].stepper.stats),
                             "replayed_growth_percent": round(100.0 * (ms["graphed_activity"] / ms["graphed"] - 1.0), 2),
                             "eager_ms_per_pass": ems, "eager_passes_timed": edone,
                             "eager_log_us": {"record": round(1e3 * (ems["record"] - ems["forward"]), 1),
                                              "log_true": round(1e3 * (ems["log_true"] - ems["forward"]), 1)},
                             "kernel_us_by_split": kernel_alone(s, args.seed)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
