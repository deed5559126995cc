"""Spike-activity log on the device for evaluation: the reference's `vis.activity` (eval_flow.py:134-136, 234-236 calls
`model(..., log=True)` on every pass and records, per sequence, the fraction of nonzero outputs of every layer -- the number the
papers report next to AEE, because it stands in for energy).

A pass appends one row of EXACT integer counts to a device log by ONE plain, capturable launch (csrc/evf_activity.hip,
evf_activity_at): per layer of `LAYERS` and per sample, the nonzero float32 elements of the network input (after norm_input) and
of the flow, and the set bits of the spike words of the seven spiking layers.  The row is named by ONE int64 word in device
memory -- the log's own for eager passes, a word of a stepper's job table under `evaluate.ResidentEvalStep` /
`evaluate.ResidentAEEStep` -- so the launch sits inside a replayed graph; nothing is read on the host until `drain()`.

    log = ActivityLog(model, B)                                    # a network on the fused FireNet engine
    out = model(event_voxel, event_cnt)
    log.record(*model.last_io())                                   # no host read, no flush beyond reading the states
    counts = log.drain()                                           # int64 [passes since the last drain, 9, B]
    batch, slots = log.fractions(counts)                           # float64 [passes, 9] and [passes, 9, B]

`ActivityCsv` appends drained passes to `activity.csv`.  Everything but `ActivityLog` runs on the host alone."""

import ctypes
import os

import numpy as np
import torch

from . import _lib
from .devlog import DeviceLog, Ring, append_csv, on_fused_engine  # noqa: F401  (Ring: its users import it from here)

LAYERS = ("0:input", "1:head", "2:G1", "3:R1a", "4:R1b", "5:G2", "6:R2a", "7:R2b", "8:pred")  # the names of model(..., log=True)
ACT_FLOAT, ACT_WORDS = 0, 1  # EVF_ACT_FLOAT / EVF_ACT_WORDS (include/evflow.h)
KINDS = (ACT_FLOAT,) + (ACT_WORDS,) * 7 + (ACT_FLOAT,)


def layer_bits(C, H, W):
    """What a sample's count of every layer is divided by: the elements of the input and of the flow, 32 channel bits per spike
    word."""
    return [C * H * W] + [32 * H * W] * 7 + [2 * H * W]


def pass_row(row, P, p):
    """The log row of pass p of the window whose step row word holds `row` (evf_activity_at: row * row_mul + row_add with
    row_mul = P, row_add = p); a negative word skips."""
    if not 0 <= p < P:
        raise _lib.EvflowError(f"pass {p} of a window of {P} passes")
    return int(row) * int(P) + int(p)


def fractions(counts, bits):
    """counts: integers [passes, layers, B]; bits[l]: what ONE sample's count of layer l is divided by ->
    (the batch-wide fraction sum_b count / (B * bits), float64 [passes, layers] -- the reference's number, the mean of the 0/1
    tensor over the whole batch --, the per-slot fractions count / bits, float64 [passes, layers, B]).  Exact integer sums and one
    float64 division each."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 3 or counts.shape[1] != len(bits):
        raise _lib.EvflowError(f"counts of shape {counts.shape}, expected [passes, {len(bits)}, B]")
    bits = np.asarray(bits, dtype=np.int64)
    if (bits < 1).any() or (counts < 0).any() or (counts > bits[None, :, None]).any():
        raise _lib.EvflowError("activity counts outside 0 .. bits")
    B = counts.shape[2]
    batch = counts.sum(axis=2).astype(np.float64) / (B * bits).astype(np.float64)[None, :]
    slots = counts.astype(np.float64) / bits.astype(np.float64)[None, :, None]
    return batch, slots


def path(model):
    """Which path reports this network's activity: "device" (ActivityLog: a network on the fused FireNet engine), "host"
    (`model(..., log=True)`: a FireNet on the general path) or None (refused).  Host only."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return None
    fused, why = on_fused_engine(model)
    if why is None:
        return None
    return "device" if fused else "host"


def refusal(model):
    """Why the device log does not serve this network (None: it does), from the host alone: the message names the alternative."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return ("the activity log counts one rank's passes: logging under data parallelism (WORLD_SIZE > 1) is not supported; run "
                "without torch.distributed.run (WORLD_SIZE=1), or drop --activity / vis.activity")
    fused, why = on_fused_engine(model)
    if why is None:
        return (f"{type(model).__name__}.forward reports \"activity\": None (as in the reference, which logs the activity of the "
                "FireNet family only): evaluate a FireNet (LIF / PLIF / XLIF / ALIF FireNet), or drop --activity / vis.activity")
    if not fused:
        return (f"[event_flow_amd] activity: {type(model).__name__} runs on the general path ({why}): its activity is not counted "
                "on the device (ActivityLog reads the spike words of the fused FireNet engine -- LIF / PLIF / XLIF / ALIF FireNets at "
                "32 channels); using model(..., log=True) on the host instead, nine reads per pass, batch-wide fractions only")
    return None


class ActivityLog:
    """Per-pass activity counts of the nine FireNet layers, logged on the device (see the module).  The log is a ring of `rows`
    rows (`devlog.DeviceLog`); a stepper that knows its number of passes sizes it for them and never wraps."""

    def __init__(self, model, B, rows=1024):
        why = refusal(model)
        if why:
            raise _lib.EvflowError(why)
        for name in ("state_buffers", "keep_io", "last_io"):
            if not hasattr(model, name):
                raise _lib.EvflowError("ActivityLog needs a model with the fused FireNet engine")
        self.model, self.B = model, int(B)
        if self.B < 1:
            raise _lib.EvflowError("ActivityLog: a batch of at least one sample")
        # uint32 words, kept as int32 (the host reads them through a uint32 view); allocated by the first pass
        self.dlog = DeviceLog(rows, None, torch.int32, -1, what="ActivityLog")
        self.rows = self.dlog.rows
        self.shape = None  # (C, H, W) of the network input, known with the first pass
        model.keep_io(True)

    def close(self):
        """Detach from the model (it stops keeping the passes' input and flow)."""
        self.model.keep_io(False)

    # ------------------------------------------------------------------ ring
    pending = property(lambda self: self.dlog.ring.pending)
    full = property(lambda self: self.dlog.ring.full)
    steps = property(lambda self: self.dlog.ring.steps)
    log = property(lambda self: self.dlog.log)

    def advance(self, n=1):
        """`n` passes were recorded through a row word of the caller's (a stepper's job table)."""
        self.dlog.ring.advance(n)

    def _allocate(self, x):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EvflowError("ActivityLog: the first pass allocates the log; record one pass eagerly before a capture")
        B, C, H, W = x.shape
        if B != self.B:
            raise _lib.EvflowError(f"ActivityLog: a batch of {B} samples, built for {self.B}")
        self.shape = (C, H, W)
        self.bits = layer_bits(C, H, W)
        self.n = [C * H * W] + [H * W] * 7 + [2 * H * W]
        self.parts = int(_lib.load().evf_activity_parts(max(self.n)))
        if self.parts < 1:
            raise _lib.EvflowError(f"evf_activity_parts refuses sources of up to {max(self.n)} elements (1 .. 2^27 - 1)")
        self.dlog.allocate((len(LAYERS), self.B, self.parts), x.device)
        self._kind = (ctypes.c_int * len(LAYERS))(*KINDS)
        self._n = (ctypes.c_int64 * len(LAYERS))(*self.n)

    # ------------------------------------------------------------------ the launch (capturable)
    def record(self, x, flow, row_word=None, row_mul=1, row_add=0):
        """The counts of the pass that just ran on `x` (the input the network saw, after norm_input) and gave `flow`: ONE
        evf_activity_at launch.  `row_word` None: the log's own device word, filled here, and the ring moves on; else the device
        address of an int64 word the caller wrote (it calls `advance()`), the row is word * row_mul + row_add."""
        x = x.detach()
        flow = flow.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        if flow.dtype != torch.float32 or not flow.is_contiguous():
            flow = flow.float().contiguous()
        if self.log is None:
            self._allocate(x)
        C, H, W = self.shape
        if tuple(x.shape) != (self.B, C, H, W) or tuple(flow.shape) != (self.B, 2, H, W):
            raise _lib.EvflowError(f"ActivityLog: input {tuple(x.shape)} / flow {tuple(flow.shape)}, built for "
                                   f"{(self.B, C, H, W)} / {(self.B, 2, H, W)}")
        states = self.model.state_buffers()
        if len(states) != 7 or any(st is None for st in states):
            raise _lib.EvflowError("ActivityLog: the model holds no recurrent state (record() follows a forward pass)")
        words = [st[1] for st in states]
        if any(z.dtype != torch.int32 or tuple(z.shape) != (self.B, H, W) for z in words):
            raise _lib.EvflowError("ActivityLog: the spike words do not match the input")
        self.dlog.use_row_word(row_word)
        self.dlog.begin()
        src = [x] + words + [flow]
        _lib.call("evf_activity_at", (ctypes.c_void_p * len(LAYERS))(*[_lib.ptr(t) for t in src]), self._kind, self._n, len(LAYERS),
                  self.B, self.dlog.row_ptr(), int(row_mul), int(row_add), self.rows, _lib.ptr(self.log))
        self.dlog.end()
        return src  # (inside a capture the caller keeps them allocated in the graph's pool)

    # ------------------------------------------------------------------ host
    def drain(self):
        """The counts of the passes recorded since the last drain, in pass order, as int64 [passes, 9, B]: one stream
        synchronise and one device -> host copy; the parts are added in int64."""
        rows = self.dlog.drain()
        if rows is None:
            return np.empty((0, len(LAYERS), self.B), dtype=np.int64)
        return rows.view(np.uint32).astype(np.int64).sum(axis=3)

    def fractions(self, counts):
        """`fractions` with this log's bits per layer."""
        if self.shape is None:
            raise _lib.EvflowError("ActivityLog: no pass recorded yet")
        return fractions(counts, self.bits)


class ActivityCsv:
    """Drained passes as `activity.csv` under `directory`: pass, new_seq, the batch-wide fraction of the nine layers and, for
    B > 1, every slot's fractions as b<k>/<layer>.  `new_seq` is 1 on a pass in front of which the loop reset the states (the
    first pass included: the states are fresh) -- where the reference restarts its `activity_log`.  The file gets its header when
    it is created and is appended to afterwards; values are printed with %.9g of their float32 rounding."""

    def __init__(self, directory, B=None):
        self.dir, self.B = directory or ".", (int(B) if B is not None else None)  # (B None: the first write's slots tell)
        self.path = os.path.join(self.dir, "activity.csv")
        self._pass = 0

    @property
    def header(self):
        B = self.B or 1
        return ["pass", "new_seq"] + list(LAYERS) + ([f"b{k}/{layer}" for k in range(B) for layer in LAYERS] if B > 1 else [])

    @staticmethod
    def _fmt(v):
        return "%.9g" % float(np.float32(v))

    def write(self, batch, slots, new_seq):
        """Append passes: batch [n, 9], slots [n, 9, B] (None: a path that reports batch-wide fractions only -- the columns stay,
        empty), new_seq[n] flags."""
        batch = np.asarray(batch, dtype=np.float64).reshape(-1, len(LAYERS))
        if self.B is None:
            self.B = int(np.shape(slots)[2]) if slots is not None else 1
        if len(new_seq) != batch.shape[0] or (slots is not None and tuple(np.shape(slots)) != (batch.shape[0], len(LAYERS), self.B)):
            raise _lib.EvflowError("ActivityCsv: batch, slots and new_seq disagree")
        lines = []
        for i, row in enumerate(batch):
            line = [self._pass, 1 if (new_seq[i] or self._pass == 0) else 0] + [self._fmt(v) for v in row]
            if self.B > 1:
                line += ["" if slots is None else self._fmt(slots[i][l][k]) for k in range(self.B) for l in range(len(LAYERS))]
            lines.append(line)
            self._pass += 1
        append_csv(self.path, self.header, lines)


class Report:
    """What the evaluation driver keeps of the drained passes: the CSV, the mean over all passes of every layer's batch-wide
    fraction and, with `per_sequence`, every slot's fractions averaged per file over the passes in which a slot read it."""

    def __init__(self, directory, B, per_sequence=False):
        self.csv = ActivityCsv(directory, B) if directory is not None else None  # (None: numbers only, no file)
        self.B = int(B)
        self.sums = np.zeros(len(LAYERS), dtype=np.float64)
        self.passes = 0
        self.per = {} if per_sequence else None  # file -> [float64 sums [9], passes]

    def add(self, batch, slots, new_seq, files=None):
        """`files[i][b]`: the file slot b reads in pass i (per_sequence)."""
        batch = np.asarray(batch, dtype=np.float64).reshape(-1, len(LAYERS))
        if self.csv is not None:
            self.csv.write(batch, slots, new_seq)
        for i, row in enumerate(batch):  # (pass order, whatever the drains: the same sums on every path)
            self.sums += row
            self.passes += 1
            if self.per is not None and slots is not None:
                for b, f in enumerate(files[i]):
                    cell = self.per.setdefault(f, [np.zeros(len(LAYERS), dtype=np.float64), 0])
                    cell[0] += np.asarray(slots[i])[:, b]
                    cell[1] += 1

    def summary(self):
        return {layer: float(self.sums[l] / max(self.passes, 1)) for l, layer in enumerate(LAYERS)}

    def into(self, out):
        """The driver's JSON: "activity", and "activity" under every file of "per_sequence"."""
        out["activity"] = self.summary()
        if self.per is not None:
            per_seq = out.setdefault("per_sequence", {})
            for f, (sums, n) in self.per.items():
                per_seq.setdefault(f, {})["activity"] = {layer: float(sums[l] / max(n, 1)) for l, layer in enumerate(LAYERS)}
        return out
