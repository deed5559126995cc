"""What does the training monitor cost per optimizer step of `train_flow.py --resident --graphed --fused-optimizer`?  c3 driver shape
(tools/driver_rate.py: LIFFireNet, B = 8 slots, 128 x 128, passes of 1000 events, P = 10 passes per step, FlatAdam), hot-pixel
filter off, every step one job-table copy and one graph launch (train.ResidentWindowStep).

Cases, each a fresh child process (one GPU process at a time), alternated round after round inside ONE call:
  parent    the parent commit's tree (--parent DIR: an export of it with its library built), no monitor
  plain     this tree, no monitor attached
  monitor   this tree, monitor.TrainMonitor attached (drained whenever its ring is about to wrap)
Reported: milliseconds per optimizer step per round (host clock around a final device synchronise), the spread the parent shows
against itself, and -- from separate profiled runs, --nodes -- the kernels of one replayed step (--count-trace on a rocprofv3
kernel trace of a child: the dispatches between the last two k_clip_adam launches, as tools/step_nodes.py counts them).

  python tools/train_monitor_rate.py --parent /path/to/parent/tree [--rounds 3] [--seconds 2] [--out profiles/train_monitor_rate.json]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/train_monitor_rate.py --child --case monitor --data D --seconds 0.3
  python tools/train_monitor_rate.py --count-trace DIR
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    root = os.path.abspath(args.root or HERE)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import numpy as np
    import torch

    from driver_rate import parts
    from loader_rate import P

    from event_flow_amd.train import ResidentWindowStep

    np.random.seed(args.seed)
    model, lossf, opt, data = parts(args.data, False, 1.0, True)
    monitor = None
    if args.case == "monitor":
        from event_flow_amd.monitor import TrainMonitor

        monitor = TrainMonitor(model, opt, rows=1024)
        stepper = ResidentWindowStep(model, lossf, opt, data, P, monitor=monitor)
    else:
        stepper = ResidentWindowStep(model, lossf, opt, data, P)

    def step():
        if monitor is not None and monitor.full:
            monitor.drain()
        stepper.step()

    for _ in range(8):  # warm-up: allocator, pinned blocks, first launches, the two graphs
        step()
    torch.cuda.synchronize()
    spent, done = 0.0, 0
    while spent < args.seconds:
        t0 = time.perf_counter()
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        done += 8
    out = {"case": args.case, "ms_per_step": round(1e3 * spent / done, 4), "steps": done, "counters": dict(stepper.stats)}
    if monitor is not None:
        rows = monitor.drain()
        out["last_row"] = dict(zip(monitor.columns()[:3] + monitor.columns()[monitor.rate_offset:],
                                   [float(v) for v in list(rows[-1][:3]) + list(rows[-1][monitor.rate_offset:])]))
    print("RESULT " + json.dumps(out), flush=True)


def count_trace(where):
    """Kernels of ONE replayed step in the rocprofv3 kernel trace under `where`: the dispatches behind the last but one k_clip_adam
    launch up to and including the last one -> (count, {kernel name: (launches, summed us)})."""
    import csv
    import glob
    import re

    files = sorted(glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        sys.exit("no kernel trace under %s" % where)
    rows = list(csv.DictReader(open(files[-1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    adam = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_clip_adam")]
    if len(adam) < 2:
        sys.exit("fewer than two k_clip_adam dispatches in the trace")
    agg = {}
    for r in rows[adam[-2] + 1:adam[-1] + 1]:
        name = re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["Kernel_Name"]))
        c, t = agg.get(name, (0, 0.0))
        agg[name] = (c + 1, t + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return adam[-1] - adam[-2], agg


def run_child(root, case, data, seconds, seed):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--case", case, "--data", data, "--seconds", str(seconds),
           "--seed", str(seed)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default="", help="child: the tree whose event_flow_amd and tools are used")
    ap.add_argument("--case", default="plain", choices=["plain", "monitor"])
    ap.add_argument("--data", default="", help="directory of the sequence files (made from --seed when empty)")
    ap.add_argument("--parent", default="", help="an export of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per child, at least")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--events", type=int, default=150000)
    ap.add_argument("--nodes", default="", help="JSON {case: kernels of one replayed step} from the profiled runs, copied into the result")
    ap.add_argument("--count-trace", default="", help="only count the kernels of one replayed step in the rocprofv3 trace under this directory")
    ap.add_argument("--make-data", action="store_true", help="only write the sequence files into --data")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.count_trace:
        n, agg = count_trace(args.count_trace)
        print("%d kernels, busy %.3f ms (under the profiler)" % (n, sum(t for _c, t in agg.values()) / 1e3))
        for name, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print("%-60s %5d %9.1f" % (name[:60], c, t))
        return
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from loader_rate import B, H, N, P, W, make_files

    if args.make_data:
        os.makedirs(args.data, exist_ok=True)
        make_files(args.data, args.seed, args.files, args.events)
        return
    cases = ([("parent", args.parent, "plain")] if args.parent else []) + [("plain", HERE, "plain"), ("monitor", HERE, "monitor")]
    result = {"shape": {"B": B, "N": N, "H": H, "W": W, "P": P}, "model": "LIFFireNet", "unit": "ms per optimizer step",
              "driver": "--resident --graphed --fused-optimizer (ResidentWindowStep, hot-pixel filter off)", "rounds": args.rounds,
              "seconds_per_child": args.seconds, "ms_per_step": {name: [] for name, _r, _c in cases}}
    with tempfile.TemporaryDirectory() as tmp:
        data = args.data or tmp
        if not args.data:
            make_files(data, args.seed, args.files, args.events)
        for _ in range(args.rounds):
            for name, root, case in cases:
                r = run_child(root, case, data, args.seconds, args.seed)
                result["ms_per_step"][name].append(r["ms_per_step"])
                result.setdefault("steps_timed", {}).setdefault(name, []).append(r["steps"])
                if "last_row" in r:
                    result["monitor_last_row"] = r["last_row"]
    ms = result["ms_per_step"]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    result["median"] = {k: med(v) for k, v in ms.items()}
    if "parent" in ms:
        result["parent_spread"] = [min(ms["parent"]), max(ms["parent"])]
        result["plain_spread"] = [min(ms["plain"]), max(ms["plain"])]
        # (the parent against itself: its rounds' range; "within": the median of `plain` inside it -- a median BELOW the range is
        #  reported as it is, by the two flags)
        result["plain_median_within_parent_spread"] = bool(min(ms["parent"]) <= med(ms["plain"]) <= max(ms["parent"]))
        result["plain_median_above_parent_spread"] = bool(med(ms["plain"]) > max(ms["parent"]))
        result["monitor_minus_plain_ms"] = round(med(ms["monitor"]) - med(ms["plain"]), 4)
    if args.nodes:
        result["kernels_per_replayed_step"] = json.loads(args.nodes)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
