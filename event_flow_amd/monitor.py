"""Training log on the device: the reference's `vis.store_grads` (train_flow.py:159-160, utils/gradients.py: mean, min and max of
|grad| per weight tensor after clipping, every optimizer step) and the spike rate of every layer of the fused FireNets, for the
fused-optimizer steps -- eager or replayed from a hipGraph -- whose gradient cannot be read afterwards (evf_clip_adam_* clip,
apply and clear the flat gradient in one launch) and whose only output is the loss.

A step appends one row to a device log by plain, capturable launches (csrc/evf_train_log.hip); the row is named by ONE int64
word in device memory -- the monitor's own for eager steps, a word of the step's job table under `train.ResidentWindowStep`:

    [loss, grad_norm, clip_coef, (<param>_mean, <param>_min, <param>_max) per weight tensor ..., rate/<layer> ...]

    monitor = TrainMonitor(model, optimizer)                       # FlatAdam
    loss = train_window(model, loss_function, optimizer, passes, monitor=monitor)
    rows = monitor.drain()                                         # numpy [steps since the last drain, len(monitor.columns())]

`CsvLog` writes drained rows as `grads_w.csv` (the reference's `save_csv` layout) and `train_log.csv`.
"""

import ctypes
import os
import sys

import numpy as np
import torch

from . import _lib, activity
from .devlog import DeviceLog, append_csv, on_fused_engine

HEAD = ("loss", "grad_norm", "clip_coef")
LAYERS = activity.LAYERS[1:8]  # the seven spiking layers, by the names of model(..., log=True)
MAX_SLOTS = 256  # (layer, pass) spike tensors of one window (evf_spike_rates_store)


def weight_segments(model):
    """[(name, offset, numel)] of the parameters whose name contains "weight" (the reference's rule, utils/gradients.py), in
    named_parameters() order; `offset` is the parameter's place in FlatAdam's flat buffers (the trainable parameters in
    parameters() order).  Host only."""
    out, off = [], 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if "weight" in name:
            out.append((name, off, p.numel()))
        off += p.numel()
    return out


def has_spike_rates(model):
    return on_fused_engine(model)[0]


def rates_notice(model):
    """What the monitor says once about a network whose spike rates it cannot log (None: it logs them)."""
    fused, why = on_fused_engine(model)
    if fused:
        return None
    why = "no FireNet-family network" if why is None else why
    return (f"[event_flow_amd] TrainMonitor: {type(model).__name__} runs on the general path ({why}): gradient statistics only, no "
            "rate/<layer> columns -- spike rates are counted from the spike words of the fused FireNet engine (LIF / PLIF / XLIF / "
            "ALIF FireNets at 32 channels); model(..., log=True) reports a general-path network's activity pass by pass")


def grad_columns(model):
    return [f"{name}_{stat}" for name, _off, _n in weight_segments(model) for stat in ("mean", "min", "max")]


def rate_columns(model):
    return [f"rate/{layer}" for layer in LAYERS] if has_spike_rates(model) else []


def columns(model):
    """The names of a log row's floats, in order."""
    return list(HEAD) + grad_columns(model) + rate_columns(model)


def refusal(optimizer=None, fused_optimizer=None, want_rates=False):
    """Why the device monitor cannot serve this call (None: it can), from the host alone: the message names the alternative."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return ("the training monitor logs one rank's step: logging under data parallelism (WORLD_SIZE > 1) is not supported; run "
                "without torch.distributed.run (WORLD_SIZE=1), or drop --monitor / vis.store_grads")
    if fused_optimizer is False and want_rates:
        return ("--monitor's spike rates are counted on the device beside the flat clip + Adam step: add --fused-optimizer (without it "
                "only vis.store_grads is served, by utils.gradients.get_grads on the host)")
    if optimizer is not None and not (hasattr(optimizer, "flat_grad") and hasattr(optimizer, "norm_ws")):
        return (f"TrainMonitor needs train.FlatAdam (the flat gradient buffer and the norm its step kernel leaves), not "
                f"{type(optimizer).__name__}: build the optimizer with FlatAdam (--fused-optimizer), or use "
                "utils.gradients.get_grads on the host after clip_grad_norm_")
    return None


class TrainMonitor:
    """Gradient statistics and spike rates of every optimizer step, logged on the device (see the module).

    The log is a ring of `rows` rows (`devlog.DeviceLog`): the owner drains before the ring wraps (`pending`, `full`).  Spike
    rates exist only for a network on the fused FireNet engine (`model.compute_path[0] == "fused"`); on the
    general path the monitor logs gradients only and says so once."""

    def __init__(self, model, optimizer, rows=1024):
        why = refusal(optimizer=optimizer)
        if why:
            raise _lib.EvflowError(why)
        self.model, self.opt = model, optimizer
        self.segments = weight_segments(model)
        if not self.segments:
            raise _lib.EvflowError("TrainMonitor: the model has no trainable parameter whose name contains 'weight'")
        if sum(p.numel() for p in model.parameters() if p.requires_grad) != optimizer.n:
            raise _lib.EvflowError("TrainMonitor: the optimizer's flat buffers do not hold this model's parameters")
        self._columns = columns(model)
        self.rates = has_spike_rates(model)
        if not self.rates:
            print(rates_notice(model), file=sys.stderr)
        self.row_floats = len(self._columns)
        self.rate_offset = len(HEAD) + 3 * len(self.segments)
        dev = optimizer.flat_grad.device
        lib = _lib.load()
        self.nseg = len(self.segments)
        self.max_n = max(n for _name, _off, n in self.segments)
        self.dlog = DeviceLog(rows, (self.row_floats,), torch.float32, float("nan"), dev, "TrainMonitor")
        self.rows, self.log = self.dlog.rows, self.dlog.log
        self.seg_off = torch.tensor([off for _name, off, _n in self.segments], dtype=torch.int64, device=dev)
        self.seg_n = torch.tensor([n for _name, _off, n in self.segments], dtype=torch.int64, device=dev)
        need = int(lib.evf_grad_stats_ws(self.nseg, self.max_n))
        if need < 0:
            raise _lib.EvflowError(f"evf_grad_stats_ws({self.nseg}, {self.max_n}) failed with status {need}")
        self.grad_ws = torch.empty(need, dtype=torch.float32, device=dev)
        self.spike_ws = torch.empty((MAX_SLOTS, int(lib.evf_spike_count_parts())), dtype=torch.int32, device=dev) if self.rates else None
        self._slot_layer = None  # the window's counted slots, between count_spikes and after_step
        if self.rates:
            model._eng()._spike_taps = []

    def close(self):
        """Detach from the model's engine (it stops collecting the windows' spike words)."""
        eng = getattr(self.model, "_engine", None)
        if eng is not None:
            eng._spike_taps = None

    def columns(self):
        return list(self._columns)

    # ------------------------------------------------------------------ ring and row word (the log's)
    pending = property(lambda self: self.dlog.ring.pending)
    full = property(lambda self: self.dlog.ring.full)
    steps = property(lambda self: self.dlog.ring.steps)

    def use_row_word(self, ptr):
        """The row of every following step is read from the int64 word at device address `ptr` (a word of the step's job table,
        written by the stepper, which also calls `advance()`); None: back to the monitor's own word."""
        self.dlog.use_row_word(ptr)

    def next_row(self):
        """The row the next step fills.  Raises when that row still holds a step that was not drained."""
        return self.dlog.ring.next_row()

    def advance(self):
        self.dlog.ring.advance()

    # ------------------------------------------------------------------ launches (all capturable)
    def begin_window(self):
        """In front of the window's first pass: spike words an earlier, abandoned window left behind are dropped."""
        if self.rates:
            self.model._eng()._spike_taps = []

    def count_spikes(self):
        """After the window's forward has been flushed, before its backward: evf_spike_count on the spike words the engine
        collected, 32 sources a launch; the list is dropped."""
        if not self.rates:
            return
        eng = self.model._eng()
        taps, eng._spike_taps = eng._spike_taps, []
        if not taps:
            raise _lib.EvflowError("TrainMonitor: the window recorded no pass (the monitor counts the spike words of training passes)")
        if len(taps) > MAX_SLOTS:
            raise _lib.EvflowError(f"TrainMonitor: {len(taps)} (layer, pass) spike tensors in one window, at most {MAX_SLOTS} "
                                   f"({MAX_SLOTS // len(LAYERS)} passes)")
        n_words = taps[0][1].numel()
        if any(z.numel() != n_words or z.dtype != torch.int32 for _l, z in taps):
            raise _lib.EvflowError("TrainMonitor: the window's spike tensors differ in size")
        for lo in range(0, len(taps), 32):
            part = taps[lo:lo + 32]
            _lib.call("evf_spike_count", (ctypes.c_void_p * 32)(*[_lib.ptr(z) for _l, z in part]), len(part), n_words,
                      _lib.ptr(self.spike_ws), lo, MAX_SLOTS)
        self._slot_layer = [layer for layer, _z in taps]
        per_layer = {layer: self._slot_layer.count(layer) for layer in range(len(LAYERS))}
        if len(set(per_layer.values())) != 1:
            raise _lib.EvflowError("TrainMonitor: the layers recorded different numbers of passes")
        self._total_bits = per_layer[0] * n_words * 32

    def before_step(self):
        """Before `optimizer.step()`, which clears the gradient: evf_grad_stats_partial."""
        self.dlog.begin()
        _lib.call("evf_grad_stats_partial", _lib.ptr(self.opt.flat_grad), _lib.ptr(self.seg_off), _lib.ptr(self.seg_n), self.nseg,
                  self.max_n, _lib.ptr(self.grad_ws), self.grad_ws.numel())

    def after_step(self, loss):
        """After `optimizer.step()`, so that the logged norm and coefficient are the applied ones: evf_grad_stats_store and
        evf_spike_rates_store into the step's row."""
        row = self.dlog.row_ptr()
        clip = self.opt.clip
        _lib.call("evf_grad_stats_store", _lib.ptr(self.grad_ws), self.grad_ws.numel(), _lib.ptr(self.seg_n), self.nseg, self.max_n,
                  _lib.ptr(self.opt.norm_ws), float(clip) if clip is not None else 0.0,
                  _lib.ptr(loss.detach().view(1)) if loss is not None else None, row, self.rows, _lib.ptr(self.log),
                  self.row_floats, 0)
        if self.rates:
            if self._slot_layer is None:
                raise _lib.EvflowError("TrainMonitor: window_apply without window_backward(monitor=...): no spike counts for this step")
            sl, self._slot_layer = self._slot_layer, None
            _lib.call("evf_spike_rates_store", _lib.ptr(self.spike_ws), MAX_SLOTS, (ctypes.c_int * MAX_SLOTS)(*sl), len(sl),
                      len(LAYERS), self._total_bits, row, self.rows, _lib.ptr(self.log), self.row_floats, self.rate_offset)
        self.dlog.end()

    # ------------------------------------------------------------------ host
    def drain(self):
        """The rows written since the last drain, in step order, as a numpy array [n, len(columns())]: one device -> host copy
        behind a stream synchronise."""
        rows = self.dlog.drain()
        return rows if rows is not None else np.empty((0, self.row_floats), dtype=np.float32)


class CsvLog:
    """The drained rows of a monitor as two files under `directory`: `grads_w.csv` -- the reference's `save_csv` layout, an index
    column with the step within the epoch and then <param>_mean, <param>_min, <param>_max, read back by
    `pandas.read_csv(index_col=0)` -- and `train_log.csv`: epoch, step, loss, grad_norm, clip_coef, rate/<layer> ...  A file gets
    its header when it is created and is appended to afterwards; values are printed with %.9g, which a float32 survives."""

    def __init__(self, directory, names):
        self.dir = directory or "."
        names = list(names)
        self.grad_idx = [i for i, c in enumerate(names) if c not in HEAD and not c.startswith("rate/")]
        self.log_idx = [i for i, c in enumerate(names) if c in HEAD or c.startswith("rate/")]
        self.grad_header = [""] + [names[i] for i in self.grad_idx]
        self.log_header = ["epoch", "step"] + [names[i] for i in self.log_idx]
        self._epoch, self._step = None, 0

    @staticmethod
    def _fmt(v):
        return "%.9g" % float(v)

    def write(self, epoch, rows):
        """Append `rows` (numpy [n, len(names)], the steps of `epoch` in order); the step index restarts with every epoch."""
        if epoch != self._epoch:
            self._epoch, self._step = epoch, 0
        grads, logs = [], []
        for r in np.asarray(rows):
            grads.append([self._step] + [self._fmt(r[i]) for i in self.grad_idx])
            logs.append([epoch, self._step] + [self._fmt(r[i]) for i in self.log_idx])
            self._step += 1
        if grads and self.grad_idx:
            append_csv(os.path.join(self.dir, "grads_w.csv"), self.grad_header, grads)
        if logs and self.log_idx:
            append_csv(os.path.join(self.dir, "train_log.csv"), self.log_header, logs)
