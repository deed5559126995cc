"""Graph-replayed evaluation on device-resident sequences (eval_flow.py --resident --graphed): one evaluated window --
P = ceil(window_eval / window) forward passes, the sharpness of every pass' image of warped events and FWL / RSAT over the
window -- as one pinned -> device copy of an extended job table plus one hipGraph launch, with the results appended to a
device log that the host reads ONCE, at the end (csrc/evf_eval_log.hip).  FWL / RSAT in `data.mode: events` only: there every
batch adds exactly `window` events, so the metric cadence is fixed and the plan (dataloader.resident.ResidentPlan.plan_eval_steps)
is host-only (`ResidentEvalStep`).  AEE alone in the ground-truth modes gtflow_dt1 / gtflow_dt4 uses only the last pass of a
ground-truth interval, and which passes close one is host-known (dataloader.resident_eval.ResidentEvalPlan.plan_eval_passes): there
the replay unit is a PASS (`ResidentAEEStep`, evf_aee_at).  The per-sequence accumulator and the log's reduction below need no
device."""

import ctypes
import os

import numpy as np
import torch

from . import _lib
from .dataloader.resident import ResidentWindow, zero_states_if
from .devlog import on_fused_engine
from .utils.iwe import compute_pol_iwe

AEE_MODES = ("gtflow_dt1", "gtflow_dt4")  # the ground-truth modes: AEE alone is replayed pass by pass (ResidentAEEStep)


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
    names = list(config.get("metrics", {}).get("name", []))
    if mode in AEE_MODES and names == ["AEE"]:  # AEE alone on ground-truth windows: a graph launch per pass (ResidentAEEStep)
        if config.get("loss", {}).get("overwrite_intermediate", False):
            return ("--graphed evaluates AEE on the flow and the event mask of the pass that closes a ground-truth interval; with "
                    "loss.overwrite_intermediate AEE needs the union of the event masks over the interval's passes: use --resident "
                    "without --graphed")
    elif mode != "events":
        return (f"--graphed serves data.mode 'events', and AEE alone (metrics.name [AEE]) in the ground-truth modes, not '{mode}' "
                f"with metrics {names}: windows by time, frame or ground-truth map have ragged widths and an irregular metric "
                "cadence (FWL / RSAT beside AEE among them), which stay on the eager path: use --resident without --graphed")
    elif "AEE" in names:
        return ("--graphed evaluates FWL / RSAT in data.mode 'events'; AEE needs a ground-truth mode (gtflow_dt1 / gtflow_dt4 with "
                "metrics.name [AEE]): drop --graphed")
    if model is not None:
        fused, why = on_fused_engine(model)
        if not fused:
            return (f"--graphed needs a network on the fused FireNet engine; {type(model).__name__} runs on the general path "
                    f"({'no fused FireNet engine' if why is None else why}): use --resident without --graphed")
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


def sum_metric_rows(out, host, names, B, row_files=None):
    """Into `out`: per metric k of `names` the logged batch means host[r][k * (B + 1) + B] summed as Python floats in row order
    and divided by max(rows, 1); `row_files[r][b]`: the file slot b reads at row r -> the per-slot values by file as
    "per_sequence" as well.  `host`: the rows as lists of Python floats."""
    per = PerSequence() if row_files is not None else None
    for k, name in enumerate(names):
        total = 0.0
        for r, row in enumerate(host):
            total += row[k * (B + 1) + B]
            if per is not None:
                per.add(name, row_files[r], row[k * (B + 1):k * (B + 1) + B])
        out[name] = total / max(len(host), 1)
    if per is not None:
        out["per_sequence"] = per.summary()
    return out


def reduce_eval_log(log, tail_sharp, names, B, P, row_files=None):
    """The eager driver's accumulation over a result log [rows, row_layout(K, B, P)] (float32, any device) and the sharpness
    scalars of the tail passes (float32 [n], same device): the metrics are summed as Python floats in row order from the
    logged batch means and divided by max(rows, 1); iwe_variance is the mean of ONE contiguous float32 vector of all sharpness
    scalars in pass order, taken on the log's device (torch.stack([...]).mean() of the eager loop).  `row_files[r][b]`: the file
    slot b reads at row r -> "per_sequence" as well.  ONE device -> host read of the log."""
    K = len(names)
    if log.shape[1] != row_layout(K, B, P):
        raise _lib.EvflowError(f"result log rows of {log.shape[1]} floats, expected {row_layout(K, B, P)}")
    sharp = torch.cat([log[:, K * (B + 1):].reshape(-1), tail_sharp.reshape(-1).to(log.dtype)])
    return sum_metric_rows({"iwe_variance": float(sharp.mean())}, log.cpu().tolist(), names, B, row_files)


class _ReplayedSteps:
    """What the replayed evaluation steppers share: two alternately replayed graphs of `self._launches(None)` -- graph A starts
    from the state tensors the warm-up left and ends in tensors of its own pool, graph B starts from those and writes its last
    pass straight back (FireNet.final_states_into), so the recurrent state crosses replays without a copy -- and the step
    itself: the table copy, then the launches eagerly (the first `warmup` steps, `replay=False`) or one graph launch."""

    def _init_replay(self, model, warmup, replay):
        what = type(self).__name__
        for name in ("state_buffers", "set_state_buffers", "final_states_into", "mark_last_pass"):
            if not hasattr(model, name):
                raise _lib.EvflowError(f"{what} needs a model with the fused FireNet engine")
        fused, why = on_fused_engine(model)
        if not fused:
            raise _lib.EvflowError(f"{what} needs a network on the fused FireNet engine ({why})")
        self.model, self.replay = model, bool(replay)
        self.warmup, self.seen = max(int(warmup), 2), 0
        self.stream = torch.cuda.Stream()
        self.graphs = None
        self.stats = {"eager": 0, "replayed": 0, "replayed_reset": 0, "graph_a": 0, "graph_b": 0}

    def _init_activity(self, activity, per_sequence, passes):
        """`activity`: an activity.ActivityLog (None: nothing changes) whose one launch follows every forward, inside the
        captured graphs as well; the log is sized for the `passes` the host knows of (None: the caller vouches), not a ring."""
        self.activity, self.activity_report = activity, None
        self.pass_new = []  # per recorded pass: the loop reset the states in front of it
        self.pass_files = [] if (activity is not None and per_sequence) else None  # ... and the file every slot reads
        self._activity_out = None
        if activity is None:
            return
        if activity.B != self.B or activity.model is not self.model:
            raise _lib.EvflowError(f"{type(self).__name__}: the activity log serves another model or batch size")
        if passes is not None and activity.rows < passes:
            raise _lib.EvflowError(f"{type(self).__name__}: an activity log of {activity.rows} rows for {passes} passes")

    def _activity_results(self, out, per_sequence):
        """ "activity" (and "activity" under every file of "per_sequence") into `out`: the log's one host read."""
        if self.activity is None:
            return out
        if self._activity_out is None:
            from .activity import Report

            report = self.activity_report if self.activity_report is not None else Report(None, self.B, per_sequence)
            batch, slots = self.activity.fractions(self.activity.drain())
            report.add(batch, slots, self.pass_new, self.pass_files)
            self._activity_out = report
        return self._activity_out.into(out)

    def _capture(self):
        home = self.model.state_buffers()
        if any(st is None for st in home):
            raise _lib.EvflowError(f"{type(self).__name__}: the model holds no recurrent state to capture from (warmup >= 1 eager step)")
        self.graphs = []
        for gi in range(2):
            if gi == 1:
                self.model.final_states_into(home)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream, capture_error_mode="global"):
                keep = self._launches(None)
            # (`keep`: the step's buffers and the sources of the row stay allocated in the graph's pool)
            self.graphs.append((g, self.model.state_buffers(), keep))

    def _step(self, send, reset, any_reset):
        """Step `self.seen`: `send()` stages and copies its table, then `self._launches(reset)` eagerly or one graph launch
        (`any_reset`: the table asks the replayed graph for a zero-fill of the state)."""
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream), torch.no_grad():
            send()
            if not self.replay or self.seen < self.warmup:
                self._launches(reset)
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
                self.stats["replayed_reset"] += 1 if any_reset else 0
                self.stats["graph_b" if gi else "graph_a"] += 1
            self.seen += 1
        cur.wait_stream(self.stream)


class ResidentEvalStep(_ReplayedSteps):
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
    `activity`: an `activity.ActivityLog` of at least as many rows as the loop has passes -- its one launch follows every forward,
    inside both graphs too (row = step row * P + p; the tail through the log's own word), and `results()` gains "activity".

        stepper = ResidentEvalStep(model, criteria, names, loader, P, rows, flow_scaling)
        for group, pass_reset, tail in loader.plan_eval_steps(P):
            stepper.step_tail(group, pass_reset) if tail else stepper.step(group, pass_reset)
        out = stepper.results()
    """

    def __init__(self, model, criteria, names, loader, P, rows, flow_scaling, overwrite_intermediate=False, warmup=2,
                 replay=True, per_sequence=False, activity=None):
        for name in ("plan_eval_steps", "_job_table", "_launch_cut"):
            if not hasattr(loader, name):
                raise _lib.EvflowError("ResidentEvalStep needs a ResidentLoader (the windows are cut out of its device-resident arena)")
        self._init_replay(model, warmup, replay)
        self.criteria, self.names, self.loader = list(criteria), list(names), loader
        self.P, self.rows = int(P), int(rows)
        self.flow_scaling, self.overwrite = flow_scaling, bool(overwrite_intermediate)
        B, P, K = loader.batch_size, self.P, len(self.names)
        self.B, self.K = B, K
        extra = (P + 1) // 2 + 1  # behind the job table: P int32 pass_reset words (a whole int64 word), the row word
        self.window = ResidentWindow(loader, P, extra_words=extra)
        self._reset_flags = self.window.table_dev.data_ptr() + 8 * self.window.base
        self._row_word = self._reset_flags + 8 * (extra - 1)
        self.row_floats = row_layout(K, B, P)
        self.log = torch.full((max(self.rows, 1), self.row_floats), float("nan"), dtype=torch.float32, device=loader.device)
        self.tail_sharp = []  # 0-d tensors of the tail passes
        self.row_files = [] if per_sequence else None
        self.stats["tail_passes"] = 0
        self._init_activity(activity, per_sequence, self.rows * P)

    # ------------------------------------------------------------------ launches
    def _passes(self, passes, pass_reset, own_row=False):
        """Forward, image of warped events, sharpness scalar and association of every pass -> (sharpness scalars, last flow).
        `pass_reset` None: a captured graph, the state tensors the pass reads are zero-filled under its word of the table; else
        the eager reset.  With an activity log: its launch behind every forward, into row (step row) * P + p, or (`own_row`, the
        tail) into the row of the log's own word."""
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
            if self.activity is not None:
                if own_row:
                    self.activity.record(*self.model.last_io())
                else:
                    self.activity.record(*self.model.last_io(), row_word=self._row_word, row_mul=self.P, row_add=p)
            iwe = compute_pol_iwe(x["flow"][-1], d["event_list"], res, d["event_list_pol_mask"][:, :, 0:1],
                                  d["event_list_pol_mask"][:, :, 1:2], flow_scaling=self.flow_scaling, round_idx=True)
            sharp.append(iwe.sum(1).var(dim=(1, 2)).mean())
            for metric in self.criteria:
                metric.event_flow_association(x["flow"], d)
        return sharp, x

    def _launches(self, pass_reset):
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

        def send():
            extra = self.window.stage(group, self.seen)
            extra[:-1] = 0
            extra[:-1].view(np.int32)[:self.P] = [1 if r else 0 for r in pass_reset]
            extra[-1] = row
            self.window.send()

        self._step(send, list(pass_reset), any(pass_reset))
        self._note_passes(group, pass_reset)
        if self.activity is not None:
            self.activity.advance(self.P)
        if self.row_files is not None:  # the file every slot reads in the window's last batch, where the loop evaluates
            self.row_files.append([os.path.basename(path) for path, _first, _flags, _restarted in group[-1][0]])

    def _note_passes(self, group, pass_reset):
        if self.activity is None:
            return
        self.pass_new += [bool(r) for r in pass_reset]
        if self.pass_files is not None:
            self.pass_files += [[os.path.basename(job[0]) for job in jobs] for jobs, _restarted, _done in group]

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
            sharp, _x = self._passes(self.loader.window_passes(group), list(pass_reset), own_row=True)
            self._note_passes(group, pass_reset)
            self.tail_sharp += sharp
            self.stats["tail_passes"] += len(group)
        cur.wait_stream(self.stream)

    def results(self):
        """The eager driver's numbers from the log (`reduce_eval_log`): the one host read of the evaluation."""
        torch.cuda.current_stream().wait_stream(self.stream)
        log = self.log[:self.seen]
        tail = torch.stack(self.tail_sharp) if self.tail_sharp else torch.empty(0, dtype=torch.float32, device=self.log.device)
        return self._activity_results(reduce_eval_log(log, tail, self.names, self.B, self.P, self.row_files), self.row_files is not None)


class ResidentAEEStep(_ReplayedSteps):
    """One pass of eval_flow.py's AEE evaluation on ground-truth windows (`data.mode` gtflow_dt1 / gtflow_dt4, metrics [AEE],
    no overwrite_intermediate) on a `ResidentEvalLoader` as one pinned -> device copy plus one graph launch.  AEE uses only the
    flow, the event mask and the ground-truth map of the pass that closes a ground-truth interval, so nothing accumulates
    across passes and the replay unit is a PASS; which passes evaluate is the host's knowledge (`plan_eval_passes`).

    The copied table is `ResidentEvalLoader._job_table(jobs)`, then ONE int32 reset word (in an int64 word), the int64 row of
    the sharpness log this pass fills, and the int64 row of the AEE log -- -1 on a pass that does not evaluate, which
    evf_aee_at answers by storing nothing.  Each of the two graphs (`_ReplayedSteps`) holds: the loader's launches at
    `capacity` width (`ResidentEvalWindow.launch`), evf_zero_segments_if on the reset word (the loop's
    `model.reset_states()`), the forward under no_grad, compute_pol_iwe, the sharpness scalar stored by
    evf_store_segments_at under the pass row, and evf_aee_at under the AEE row.  The first `warmup` passes and every pass with
    `replay=False` run the same launches eagerly with `model.reset_states()` in place of the zero-fill.  No step reads a
    device value on the host; `results()` reads the two logs once.  `activity`: an `activity.ActivityLog` of `passes` rows -- its
    one launch follows the forward under the pass row, inside both graphs too, and `results()` gains "activity".

        plan = list(loader.plan_eval_passes())
        capacity = max([job[2] for jobs, _r, _e in plan for job in jobs] + [1])
        stepper = ResidentAEEStep(model, loader, len(plan), sum(e for _j, _r, e in plan), capacity, flow_scaling)
        for jobs, restarted, evaluate in plan:
            stepper.step(jobs, restarted, evaluate)
        out = stepper.results()
    """

    def __init__(self, model, loader, passes, evaluations, capacity, flow_scaling, warmup=2, replay=True, per_sequence=False,
                 activity=None):
        for name in ("plan_eval_passes", "_job_table", "_launch"):
            if not hasattr(loader, name):
                raise _lib.EvflowError("ResidentAEEStep needs a ResidentEvalLoader (the windows are cut out of its device-resident "
                                       "arena)")
        if loader.mode not in AEE_MODES:
            raise _lib.EvflowError(f"ResidentAEEStep evaluates AEE on ground-truth windows ({' / '.join(AEE_MODES)}), not in "
                                   f"data.mode '{loader.mode}'")
        from .dataloader.resident_eval import ResidentEvalWindow

        self._init_replay(model, warmup, replay)
        self.loader, self.flow_scaling = loader, flow_scaling
        self.passes, self.evaluations, self.B = int(passes), int(evaluations), loader.batch_size
        self.window = ResidentEvalWindow(loader, capacity, extra_words=3)
        self._reset_word = self.window.table_dev.data_ptr() + 8 * self.window.base
        self._pass_row, self._aee_row = self._reset_word + 8, self._reset_word + 16
        dev = loader.device
        self.row_floats = 2 * (self.B + 1)  # [aee_0 .. aee_{B-1}, mean, percent_0 .. percent_{B-1}, mean]
        self.sharp_log = torch.full((max(self.passes, 1),), float("nan"), dtype=torch.float32, device=dev)
        self.aee_log = torch.full((max(self.evaluations, 1), self.row_floats), float("nan"), dtype=torch.float32, device=dev)
        stripes = _lib.load().evf_aee_at_stripes(*loader.res)
        if stripes < 1:
            raise _lib.EvflowError(f"evf_aee_at_stripes refuses a resolution of {tuple(loader.res)}")
        self.ws = torch.empty(self.B * stripes * 3, dtype=torch.float32, device=dev)
        self.evaluated = 0
        self.row_files = [] if per_sequence else None
        self._init_activity(activity, per_sequence, self.passes)

    def _launches(self, reset):
        """The launches of one pass on the static buffers (see the class) -> what must stay allocated.  `reset` None: a
        captured graph, the state tensors are zero-filled under the reset word of the table; else the eager reset."""
        B = self.B
        H, W = self.loader.res
        d = self.window.launch()
        if reset is None:
            zero_states_if(self._reset_word, self.model.state_buffers())
        elif reset:
            self.model.reset_states()
        self.model.mark_last_pass()  # (every pass ends its graph: the next one starts from the state it leaves)
        x = self.model(d["event_voxel"], d["event_cnt"])
        if self.activity is not None:  # (its launch: the pass row of the table names the log's row, too)
            self.activity.record(*self.model.last_io(), row_word=self._pass_row)
        iwe = compute_pol_iwe(x["flow"][-1], d["event_list"], self.loader.res, d["event_list_pol_mask"][:, :, 0:1],
                              d["event_list_pol_mask"][:, :, 1:2], flow_scaling=self.flow_scaling, round_idx=True)
        sharp = iwe.sum(1).var(dim=(1, 2)).mean().to(torch.float32).view(1)
        _lib.call("evf_store_segments_at", self._pass_row, self.sharp_log.shape[0], _lib.ptr(self.sharp_log), 1,
                  (ctypes.c_void_p * 32)(_lib.ptr(sharp)), (ctypes.c_int * 32)(0), (ctypes.c_int * 32)(1), 1)
        flow = x["flow"][-1].detach().to(torch.float32).contiguous()
        gt = d["gtflow"].to(torch.float32).contiguous()
        mask = d["event_mask"].to(torch.float32).contiguous()
        _lib.call("evf_aee_at", _lib.ptr(flow), _lib.ptr(gt), _lib.ptr(mask), _lib.ptr(d["dt_gt"]), _lib.ptr(d["dt_input"]), B, H, W,
                  float(self.flow_scaling), self._aee_row, self.aee_log.shape[0], _lib.ptr(self.aee_log), self.row_floats, 0,
                  _lib.ptr(self.ws), self.ws.numel())
        return d, sharp, flow, gt, mask

    def step(self, jobs, restarted, evaluate):
        """One pass: a triple of `ResidentEvalPlan.plan_eval_passes`."""
        row = self.seen
        if row >= self.passes:
            raise _lib.EvflowError(f"ResidentAEEStep: pass {row} of logs sized for {self.passes} passes")
        if evaluate and self.evaluated >= self.evaluations:
            raise _lib.EvflowError(f"ResidentAEEStep: evaluation {self.evaluated} of a log sized for {self.evaluations}")

        def send():
            extra = self.window.stage(jobs, self.seen)
            extra[0] = 1 if restarted else 0
            extra[1] = row
            extra[2] = self.evaluated if evaluate else -1
            self.window.send()

        self._step(send, bool(restarted), bool(restarted))
        if self.activity is not None:
            self.activity.advance()
            self.pass_new.append(bool(restarted))
            if self.pass_files is not None:
                self.pass_files.append([os.path.basename(job[0]) for job in jobs])
        if evaluate:
            self.evaluated += 1
            if self.row_files is not None:  # the file every slot reads in the pass where the loop evaluates
                self.row_files.append([os.path.basename(job[0]) for job in jobs])

    def results(self):
        """The eager driver's numbers from the two logs, read once: AEE and AEE_percent_outliers summed as Python floats in row
        order from the logged batch means and divided by max(it, 1); iwe_variance the mean of the one contiguous float32 vector
        of the passes' sharpness scalars, taken on the device; with `per_sequence` the per-slot values by file."""
        torch.cuda.current_stream().wait_stream(self.stream)
        out = {"iwe_variance": float(self.sharp_log[:self.seen].mean())}
        sum_metric_rows(out, self.aee_log[:self.evaluated].cpu().tolist(), ("AEE", "AEE_percent_outliers"), self.B, self.row_files)
        return self._activity_results(out, self.row_files is not None)
