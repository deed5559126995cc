"""Graph-replayed evaluation on device-resident sequences (eval_flow.py --resident --graphed): one evaluated window --
P = ceil(window_eval / window) forward passes, the sharpness of every pass' image of warped events and FWL / RSAT over the
window -- as one pinned -> device copy of an extended job table plus one hipGraph launch, with the results appended to a
device log that the host reads ONCE, at the end (csrc/evf_eval_log.hip).  `data.mode: events` only: there every batch adds
exactly `window` events, so the metric cadence is fixed and the plan (dataloader.resident.ResidentPlan.plan_eval_steps) is
host-only.  The per-sequence accumulator and the log's reduction below need no device."""

import ctypes
import os

import numpy as np
import torch

from . import _lib
from .dataloader.resident import ResidentWindow, zero_states_if
from .utils.iwe import compute_pol_iwe


def graphed_refusal(args, config, model=None):
    """Why eval_flow.py --graphed does not serve these arguments / this configuration / this network (None: it does).
    Host-only: asked before any device work; every answer names the alternative."""
    if not getattr(args, "resident", False):
        return ("--graphed replays the evaluation on device-resident sequences: add --resident (without --graphed the "
                "evaluation runs eagerly on H5Loader)")
    if getattr(args, "synthetic", False):
        return "--graphed reads sequence files through the resident loader, not the synthetic one: drop --synthetic or --graphed"
    if getattr(args, "store", ""):
        return "--graphed keeps every result on the device until the end and stores no images: drop --graphed to use --store"
    mode = config["data"]["mode"]
    if mode != "events":
        return (f"--graphed serves data.mode 'events' only, not '{mode}': windows by time, frame or ground-truth map have ragged "
                "widths and an irregular metric cadence (AEE among them), which stay on the eager path: use --resident without "
                "--graphed")
    if "AEE" in config.get("metrics", {}).get("name", []):
        return "--graphed evaluates FWL / RSAT; AEE needs a ground-truth mode, which stays on the eager path: drop --graphed"
    if model is not None:
        path = getattr(model, "compute_path", ("general", "no fused FireNet engine"))
        if path[0] != "fused":
            return (f"--graphed needs a network on the fused FireNet engine; {type(model).__name__} runs on the general path "
                    f"({path[1]}): use --resident without --graphed")
    return None


def slot_files(data):
    """File name of the sequence every batch slot reads right now (the reference's
    data.files[data.batch_idx[b] % len(data.files)].split("/")[-1], eval_flow.py:184)."""
    return [os.path.basename(data.files[data.batch_idx[b] % len(data.files)]) for b in range(data.batch_size)]


class PerSequence:
    """Per-file accumulation of the metrics (reference eval_flow.py:183-199, 246-258): a slot's value goes to the file that slot
    reads at the evaluation, summed as Python floats."""

    def __init__(self):
        self.sums = {}  # file -> metric -> [sum, evaluations]

    def add(self, name, files, values):
        """`values[b]`: slot b's value of metric `name` (Python floats), `files[b]`: the file it belongs to."""
        for f, v in zip(files, values):
            cell = self.sums.setdefault(f, {}).setdefault(name, [0.0, 0])
            cell[0] += float(v)
            cell[1] += 1

    def summary(self):
        out = {}
        for f, per in self.sums.items():
            out[f] = {name: s / max(it, 1) for name, (s, it) in per.items()}
            out[f]["it"] = max(it for _s, it in per.values())
        return out


def row_layout(K, B, P):
    """Floats of a log row: K metrics x (B per-slot values, then the batch mean), then the P sharpness scalars of the passes."""
    return K * (B + 1) + P


def reduce_eval_log(log, tail_sharp, names, B, P, row_files=None):
    """The eager driver's accumulation over a result log [rows, row_layout(K, B, P)] (float32, any device) and the sharpness
    scalars of the tail passes (float32 [n], same device): the metrics are summed as Python floats in row order from the
    logged batch means and divided by max(rows, 1); iwe_variance is the mean of ONE contiguous float32 vector of all sharpness
    scalars in pass order, taken on the log's device (torch.stack([...]).mean() of the eager loop).  `row_files[r][b]`: the file
    slot b reads at row r -> "per_sequence" as well.  ONE device -> host read of the log."""
    K = len(names)
    rows = log.shape[0]
    if log.shape[1] != row_layout(K, B, P):
        raise _lib.EvflowError(f"result log rows of {log.shape[1]} floats, expected {row_layout(K, B, P)}")
    sharp = torch.cat([log[:, K * (B + 1):].reshape(-1), tail_sharp.reshape(-1).to(log.dtype)])
    host = log.cpu().tolist()
    out = {"iwe_variance": float(sharp.mean())}
    per = PerSequence() if row_files is not None else None
    for k, name in enumerate(names):
        total = 0.0
        for r in range(rows):
            total += host[r][k * (B + 1) + B]
            if per is not None:
                per.add(name, row_files[r], host[r][k * (B + 1):k * (B + 1) + B])
        out[name] = total / max(rows, 1)
    if per is not None:
        out["per_sequence"] = per.summary()
    return out


class ResidentEvalStep:
    """One evaluated window of eval_flow.py's loop on a `ResidentLoader` as one pinned -> device copy plus one graph launch.

    The copied table is `ResidentLoader._job_table(group)` (2*B*P + 1 int64 words; `_launch_cut` reads only this prefix),
    then P int32 `pass_reset` words (padded to a whole int64 word), then ONE int64 word: the row of the result log this step
    fills.  Each of two alternately replayed graphs (graph A starts from the state tensors the warm-up left and ends in
    tensors of its own pool, graph B starts from those and writes its last pass straight back -- FireNet.final_states_into --
    so the recurrent state crosses replays without a copy, also when P = 1, where one graph would have to write into the
    tensors it reads) holds: the cut, the hot-pixel kernel, the binning of the P passes and the mask launches; per pass the
    conditional zero-fill of the state tensors THAT pass reads (evf_zero_segments_if on its `pass_reset` word: the loop's
    `model.reset_states()`), the forward under no_grad, compute_pol_iwe, the sharpness scalar and the criteria's
    event_flow_association; then every criterion's forward and mean, evf_store_segments_at of the row
    [K x (B per-slot values + the batch mean)] + [P sharpness scalars], and the criteria's reset.

    The first `warmup` steps, every step with `replay=False` and the tail (`step_tail`, fewer than P batches: forwarded and
    associated, never evaluated) run the same launches eagerly with `model.reset_states()` in place of the zero-fill.  No step
    reads a device value on the host; `results()` reads the log once.  The tail comes last: a replay does not follow it.

        stepper = ResidentEvalStep(model, criteria, names, loader, P, rows, flow_scaling)
        for group, pass_reset, tail in loader.plan_eval_steps(P):
            stepper.step_tail(group, pass_reset) if tail else stepper.step(group, pass_reset)
        out = stepper.results()
    """

    def __init__(self, model, criteria, names, loader, P, rows, flow_scaling, overwrite_intermediate=False, warmup=2,
                 replay=True, per_sequence=False):
        for name in ("plan_eval_steps", "_job_table", "_launch_cut"):
            if not hasattr(loader, name):
                raise _lib.EvflowError("ResidentEvalStep needs a ResidentLoader (the windows are cut out of its device-resident arena)")
        for name in ("state_buffers", "set_state_buffers", "final_states_into", "mark_last_pass"):
            if not hasattr(model, name):
                raise _lib.EvflowError("ResidentEvalStep needs a model with the fused FireNet engine")
        if getattr(model, "compute_path", ("general", ""))[0] != "fused":
            raise _lib.EvflowError(f"ResidentEvalStep needs a network on the fused FireNet engine ({model.compute_path[1]})")
        self.model, self.criteria, self.names, self.loader = model, list(criteria), list(names), loader
        self.P, self.rows, self.replay = int(P), int(rows), bool(replay)
        self.flow_scaling, self.overwrite = flow_scaling, bool(overwrite_intermediate)
        self.warmup, self.seen = max(int(warmup), 2), 0
        B, P, K = loader.batch_size, self.P, len(self.names)
        self.B, self.K = B, K
        extra = (P + 1) // 2 + 1  # behind the job table: P int32 pass_reset words (a whole int64 word), the row word
        self.window = ResidentWindow(loader, P, extra_words=extra)
        self._reset_flags = self.window.table_dev.data_ptr() + 8 * self.window.base
        self._row_word = self._reset_flags + 8 * (extra - 1)
        self.row_floats = row_layout(K, B, P)
        self.log = torch.full((max(self.rows, 1), self.row_floats), float("nan"), dtype=torch.float32, device=loader.device)
        self.stream = torch.cuda.Stream()
        self.graphs = None
        self.tail_sharp = []  # 0-d tensors of the tail passes
        self.row_files = [] if per_sequence else None
        self.stats = {"eager": 0, "replayed": 0, "replayed_reset": 0, "graph_a": 0, "graph_b": 0, "tail_passes": 0}

    # ------------------------------------------------------------------ launches
    def _passes(self, passes, pass_reset):
        """Forward, image of warped events, sharpness scalar and association of every pass -> (sharpness scalars, last flow).
        `pass_reset` None: a captured graph, the state tensors the pass reads are zero-filled under its word of the table; else
        the eager reset."""
        res = self.loader.res
        sharp, x = [], None
        for p, d in enumerate(passes):
            d.setdefault("event_voxel", None)
            if pass_reset is None:
                zero_states_if(self._reset_flags + 4 * p, self.model.state_buffers())
            elif pass_reset[p]:
                self.model.reset_states()
            if p == self.P - 1:
                self.model.mark_last_pass()
            x = self.model(d["event_voxel"], d["event_cnt"])
            iwe = compute_pol_iwe(x["flow"][-1], d["event_list"], res, d["event_list_pol_mask"][:, :, 0:1],
                                  d["event_list_pol_mask"][:, :, 1:2], flow_scaling=self.flow_scaling, round_idx=True)
            sharp.append(iwe.sum(1).var(dim=(1, 2)).mean())
            for metric in self.criteria:
                metric.event_flow_association(x["flow"], d)
        return sharp, x

    def _window(self, pass_reset):
        """The launches of one evaluated window on the static buffers (see the class) -> its passes."""
        B = self.B
        passes = self.window.launch()
        sharp, x = self._passes(passes, pass_reset)
        src, off, cnt = [], [], []
        for k, metric in enumerate(self.criteria):
            if self.overwrite:
                metric.overwrite_intermediate_flow(x["flow"])
            val = metric().to(torch.float32).contiguous().view(B)
            src += [val, val.mean().view(1)]
            off += [k * (B + 1), k * (B + 1) + B]
            cnt += [B, 1]
        for p, s in enumerate(sharp):
            src.append(s.to(torch.float32).view(1))
            off.append(self.K * (B + 1) + p)
            cnt.append(1)
        for lo in range(0, len(src), 32):
            n = len(src[lo:lo + 32])
            _lib.call("evf_store_segments_at", self._row_word, self.log.shape[0], _lib.ptr(self.log), self.row_floats,
                      (ctypes.c_void_p * 32)(*[_lib.ptr(t) for t in src[lo:lo + 32]]), (ctypes.c_int * 32)(*off[lo:lo + 32]),
                      (ctypes.c_int * 32)(*cnt[lo:lo + 32]), n)
        for metric in self.criteria:
            metric.reset()
        return passes, src

    def _capture(self):
        home = self.model.state_buffers()
        if any(st is None for st in home):
            raise _lib.EvflowError("ResidentEvalStep: the model holds no recurrent state to capture from (warmup >= 1 eager step)")
        self.graphs = []
        for gi in range(2):
            if gi == 1:
                self.model.final_states_into(home)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream, capture_error_mode="global"):
                keep = self._window(None)
            # (`keep`: the window's buffers and the sources of the row stay allocated in the graph's pool)
            self.graphs.append((g, self.model.state_buffers(), keep))

    # ------------------------------------------------------------------ steps
    def step(self, group, pass_reset):
        """One evaluated window: the P batches of `group` with their `pass_reset` flags (a triple of `plan_eval_steps`)."""
        if len(group) != self.P or len(pass_reset) != self.P:
            raise _lib.EvflowError(f"ResidentEvalStep: a window of {len(group)} batches, built for {self.P}")
        if self.stats["tail_passes"]:
            raise _lib.EvflowError("ResidentEvalStep: the tail ends the pass over the files; no window follows it")
        row = self.seen
        if row >= self.log.shape[0] or self.rows == 0:
            raise _lib.EvflowError(f"ResidentEvalStep: step {row} of a log sized for {self.rows} windows")
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream), torch.no_grad():
            extra = self.window.stage(group, self.seen)
            extra[:-1] = 0
            extra[:-1].view(np.int32)[:self.P] = [1 if r else 0 for r in pass_reset]
            extra[-1] = row
            self.window.send()
            if not self.replay or self.seen < self.warmup:
                self._window(list(pass_reset))
                self.stats["eager"] += 1
            else:
                if self.graphs is None:
                    torch.cuda.synchronize()
                    self._capture()
                gi = (self.seen - self.warmup) & 1
                g, left, _keep = self.graphs[gi]
                g.replay()
                self.model.set_state_buffers(left)  # keep model.states / eager calls consistent with the replayed step
                self.stats["replayed"] += 1
                self.stats["replayed_reset"] += 1 if any(pass_reset) else 0
                self.stats["graph_b" if gi else "graph_a"] += 1
            self.seen += 1
        cur.wait_stream(self.stream)
        if self.row_files is not None:  # the file every slot reads in the window's last batch, where the loop evaluates
            self.row_files.append([os.path.basename(path) for path, _first, _flags, _restarted in group[-1][0]])

    def step_tail(self, group, pass_reset):
        """The fewer than P batches behind the last whole window: forwarded and associated like every batch, never evaluated
        (the loop ends before `window_eval` events are collected); their sharpness scalars count."""
        if len(group) >= self.P or len(pass_reset) != len(group):
            raise _lib.EvflowError(f"ResidentEvalStep: a tail of {len(group)} batches (fewer than {self.P} expected)")
        if not group:
            return
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream), torch.no_grad():
            sharp, _x = self._passes(self.loader.window_passes(group), list(pass_reset))
            self.tail_sharp += sharp
            self.stats["tail_passes"] += len(group)
        cur.wait_stream(self.stream)

    def results(self):
        """The eager driver's numbers from the log (`reduce_eval_log`): the one host read of the evaluation."""
        torch.cuda.current_stream().wait_stream(self.stream)
        log = self.log[:self.seen]
        tail = torch.stack(self.tail_sharp) if self.tail_sharp else torch.empty(0, dtype=torch.float32, device=self.log.device)
        return reduce_eval_log(log, tail, self.names, self.B, self.P, self.row_files)
