"""Streaming inference: optical flow from events as they arrive.  `FlowStream.push(xs, ys, ts, ps)` appends the events to a device
RING (`EventRing`: the arena's four columns with a capacity instead of a length, csrc/evf_stream.hip) and runs every window of
`window` events that is complete -- consecutive, not overlapping, window k = stream events [k N, (k + 1) N), as in `data.mode:
events` -- with the launches of the evaluation drivers: the cut (evf_ring_cut, evf_seq_cut's rows bit for bit), the hot-pixel
filter, the binning, the mask launches, the conditional zero-fill of the recurrent state, the forward under no_grad and the store
of the flow and the event mask into a device ring of `slots` results.  A push is ONE pinned -> device copy and ONE launch per
appended slice (the head word travels in front of the chunk); a window is one copy of a five-word table and, behind the warm-up,
one launch of two alternately replayed graphs (evaluate._ReplayedSteps).

What the host decides needs no device value: pushes have host-known lengths, so `plan_push` -- a pure function -- slices a
push so that the ring is never overwritten ahead of an uncut window, and names every window's first event and result row.
One stream, batch size 1, fused FireNets only: see `stream_refusal`."""

import ctypes
import gc
import os

import numpy as np
import torch

from . import _lib
from .dataloader.encodings import encode_window
from .dataloader.resident import StaticTable, zero_states_if
from .devlog import on_fused_engine
from .evaluate import _ReplayedSteps

TABLE_WORDS = 5  # int64: first | appended | int32 flags, int32 hot-pixel reset | int32 state reset, pad | result row
CHUNK_RING = 4   # pinned staging chunks in flight (>= 2)


def stream_refusal(model, world_size=None):
    """Why `FlowStream` does not serve this network / this process (None: it does).  Host-only: asked before any device work;
    every answer names the eager alternative."""
    eager = "run the windows eagerly instead: dataloader.encodings.encode_event_list + model(event_voxel, event_cnt) per window"
    world = int(os.environ.get("WORLD_SIZE", "1")) if world_size is None else int(world_size)
    if world > 1:
        return (f"FlowStream serves one stream on one device, and this process is one of WORLD_SIZE = {world} ranks: run it "
                f"without torch.distributed.run (WORLD_SIZE=1), or {eager}")
    fused, why = on_fused_engine(model)
    if not fused:
        return (f"FlowStream replays the fused FireNet engine's forward; {type(model).__name__} runs on the general path "
                f"({'no fused FireNet engine' if why is None else why}): {eager}")
    for name in ("state_buffers", "set_state_buffers", "final_states_into", "mark_last_pass"):
        if not hasattr(model, name):
            return f"FlowStream needs a model with the fused FireNet engine ({type(model).__name__} has no {name}): {eager}"
    return None


def plan_push(pending, n, N, R, slots, windows=0):
    """What a push of `n` events does, decided on the host: `pending` events (< N) wait behind `windows` whole windows of N
    events in a ring of R >= N slots, and the result ring has `slots` rows.  -> a list, in launch order, of
        ("append", lo, hi)        the push's events [lo, hi) go to slots (windows * N + pending + lo + i) mod R
        ("window", k, first, row) window k is cut from stream event first = k * N on, its result goes to row k mod slots.
    A slice never overwrites an event of a window that is not cut yet: at most R - (events appended and not cut) events are
    appended at a time, then every complete window runs (the launches are ordered on one stream, so a slot is free as soon as
    its window's cut is enqueued).  A push that completes more than `slots` windows is refused: its first results would be
    overwritten before the caller saw them."""
    pending, n, N, R, slots, windows = int(pending), int(n), int(N), int(R), int(slots), int(windows)
    if N < 1 or R < N or slots < 1 or windows < 0:
        raise _lib.EvflowError(f"plan_push: a window of {N} events in a ring of {R} slots with {slots} result rows")
    if not 0 <= pending < N:
        raise _lib.EvflowError(f"plan_push: {pending} pending events behind whole windows of {N}")
    if n < 0 or n > slots * N - pending:
        raise _lib.EvflowError(f"a push of {n} events with {pending} pending completes more than {slots} windows of {N} events, "
                               f"whose results would overwrite each other in the {slots} result rows: push at most "
                               f"{slots * N - pending} events at a time (or build the stream with more slots)")
    ops, done, uncut = [], 0, pending
    while done < n:
        take = min(n - done, R - uncut)
        ops.append(("append", done, done + take))
        done, uncut = done + take, uncut + take
        while uncut >= N:
            ops.append(("window", windows, windows * N, windows % slots))
            windows, uncut = windows + 1, uncut - N
    return ops


def check_events(xs, ys, ts, ps, H, W):
    """The host checks of a push, before any copy -> (xs uint16, ys uint16, ts float64, ps uint8)."""
    cols = [np.asarray(c) for c in (xs, ys, ts, ps)]
    if any(c.ndim != 1 for c in cols) or len({len(c) for c in cols}) != 1:
        raise _lib.EvflowError(f"push: four columns of equal length, got shapes {[tuple(c.shape) for c in cols]}")
    x, y, t, p = cols
    for name, c, hi in (("xs", x, W), ("ys", y, H)):
        if c.size and not (c.dtype.kind in "iuf" and np.all(c == np.floor(c)) and c.min() >= 0 and c.max() < hi):
            raise _lib.EvflowError(f"push: {name} holds values that are no integers in [0, {hi}) (a coordinate outside the "
                                   f"{H} x {W} sensor would index the flow map out of bounds)")
    if p.size and not (p.dtype.kind in "iufb" and np.all((p == 0) | (p == 1))):
        raise _lib.EvflowError("push: ps holds polarities outside {0, 1}")
    if t.size and not (t.dtype.kind in "iuf" and np.all(np.isfinite(t))):
        raise _lib.EvflowError("push: ts holds timestamps that are not finite")
    return x.astype(np.uint16), y.astype(np.uint16), t.astype(np.float64), p.astype(np.uint8)


class EventRing:
    """The device ring of a stream: the arena's columns (`xs`, `ys` uint16, `ts` float64, `ps` uint8) with `capacity` slots,
    stream event e at slot e mod capacity; a staging buffer in device memory (the int64 head word, then one chunk laid out ts |
    xs | ys | ps) with a ring of pinned host copies, each with an event recorded after its copy; and a host mirror of the
    timestamps.  `appended`: events pushed so far -- the host always knows it."""

    def __init__(self, capacity, device):
        self.capacity = R = int(capacity)
        if R < 1:
            raise _lib.EvflowError(f"EventRing: a capacity of {capacity} events")
        _lib.load()
        if not torch.cuda.is_available() or torch.device(device).type != "cuda":
            raise _lib.EvflowError("EventRing: the events live and are cut on the MI355X only (no CPU fallback)")
        self.device = dev = torch.device(device)
        self.xs = torch.zeros(R, dtype=torch.int16, device=dev)  # (uint16 bits: torch has no arithmetic on them, none is needed)
        self.ys = torch.zeros(R, dtype=torch.int16, device=dev)
        self.ts = torch.zeros(R, dtype=torch.float64, device=dev)
        self.ps = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.stage_dev = torch.empty(8 + 13 * R, dtype=torch.uint8, device=dev)
        self.chunks = [(torch.empty(8 + 13 * R, dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(CHUNK_RING)]
        self.ts_host = np.zeros(R, dtype=np.float64)
        self.appended, self.copies = 0, 0

    def restart(self):
        """The stream index starts again at 0 (what the ring holds is out of every window's reach: `appended` guards it)."""
        self.appended = 0

    def append(self, xs, ys, ts, ps):
        """n <= capacity events (uint16, uint16, float64, uint8 host arrays) on the current stream: one pinned -> device copy
        of head word + chunk, one evf_ring_append.  The caller keeps events of uncut windows out of the way (`plan_push`)."""
        n, R = len(xs), self.capacity
        if n > R:
            raise _lib.EvflowError(f"EventRing.append: {n} events into a ring of {R}")
        if n == 0:
            return
        pinned, copied = self.chunks[self.copies % CHUNK_RING]
        copied.synchronize()  # (the copy that read this pinned chunk CHUNK_RING appends ago)
        host = pinned.numpy()
        host[:8].view(np.int64)[0] = self.appended
        host[8:8 + 8 * n].view(np.float64)[:] = ts
        host[8 + 8 * n:8 + 10 * n].view(np.uint16)[:] = xs
        host[8 + 10 * n:8 + 12 * n].view(np.uint16)[:] = ys
        host[8 + 12 * n:8 + 13 * n] = ps
        self.stage_dev[:8 + 13 * n].copy_(pinned[:8 + 13 * n], non_blocking=True)
        copied.record()
        at = self.stage_dev.data_ptr()
        _lib.call("evf_ring_append", at + 8, n, at, _lib.ptr(self.xs), _lib.ptr(self.ys), _lib.ptr(self.ts), _lib.ptr(self.ps), R)
        at = self.appended % R  # the host mirror of the timestamps
        head = min(n, R - at)
        self.ts_host[at:at + head] = ts[:head]
        self.ts_host[:n - head] = ts[head:]
        self.appended += n
        self.copies += 1


class FlowResult:
    """One window's result.  `index`: the window's number in the stream, `first`: its first event's stream index, `t_first` /
    `t_last`: its first and last timestamp (relative to the stream's t0, from the host mirror), `ready`: an event recorded behind
    the window's launches.  `flow` [2,H,W], `event_mask` [H,W] and `flow_masked` are VIEWS into the stream's result ring, ordered
    behind the window on the stream `push` was called on; once `slots` later windows have run the row is reused, and the access
    raises."""

    def __init__(self, stream, serial, row, index, first, t_first, t_last, ready):
        self._stream, self._serial, self._row = stream, serial, row
        self.index, self.first, self.t_first, self.t_last, self.ready = index, first, t_first, t_last, ready

    def _view(self):
        if self._stream._row_serial[self._row] != self._serial:
            raise _lib.EvflowError(f"FlowResult: window {self.index}'s row {self._row} of the result ring has been reused by a later "
                                   f"window (the ring holds the last {self._stream.slots} results): copy a result before pushing "
                                   "that many windows, or build the stream with more slots")
        return self._stream.results[self._row]

    @property
    def flow(self):
        return self._view()[:2]

    @property
    def event_mask(self):
        return self._view()[2]

    @property
    def flow_masked(self):
        """eval_flow.py's `flow_vis`: the flow times the event mask when the model masks its output, else the flow."""
        row = self._view()
        return row[:2] * row[2] if self._stream.model.mask else row[:2]


class _WindowTable:
    """What `StaticTable` asks of a loader, for one window a step: the device and the host table.  An object of its own, so that
    the stream and its table do not refer to each other: a stream is then freed when its last reference goes, graphs included,
    and never by the cycle collector at a moment of its choosing (inside another stream's capture, say)."""

    def __init__(self, device):
        self.device = device

    @staticmethod
    def _job_table(job):
        """The five words of one window (see TABLE_WORDS); no flips on a live stream."""
        first, appended, reset, row = job
        tab = np.zeros(TABLE_WORDS, dtype=np.int64)
        tab[0], tab[1], tab[4] = first, appended, row
        aux = tab[2:4].view(np.int32)
        aux[1] = aux[2] = 1 if reset else 0
        return tab


class FlowStream(_ReplayedSteps):
    """Flow from pushed events (see the module): one stream, batch size 1.

        stream = FlowStream(model, config, window=20000)       # config: loader.resolution, hot_filter
        for xs, ys, ts, ps in source:                          # host arrays of any length up to stream.max_push
            for r in stream.push(xs, ys, ts, ps):
                use(r.flow)                                    # device views, ordered on the current stream; r.ready.synchronize()
                                                               # before a host read of anything else
    `capacity`: slots of the event ring (default 4 windows, at least one); `slots`: rows of the result ring; `t0`: subtracted
    from every timestamp in float64 (default: the first pushed timestamp); the first `warmup` (>= 2) windows and every window
    with `replay=False` run the launches eagerly.  `push` reads no device value and does not synchronise the device: it waits
    only for the copy that last read the pinned buffer it is about to rewrite, and once, at the capture of the two graphs."""

    def __init__(self, model, config, window, capacity=None, slots=8, t0=None, warmup=2, replay=True, round_encoding=False,
                 device=None):
        why = stream_refusal(model)
        if why:
            raise _lib.EvflowError(why)
        N, slots = int(window), int(slots)
        H, W = (int(v) for v in config["loader"]["resolution"])
        R = 4 * N if capacity is None else int(capacity)
        if N < 2 or slots < 1 or R < N:
            raise _lib.EvflowError(f"FlowStream: windows of {N} events (at least 2) in a ring of {R} slots (at least one window) with "
                                   f"{slots} result rows (at least 1)")
        if H < 1 or W < 1 or H > 65535 or W > 65535 or 3 * H * W >= 2 ** 31:
            raise _lib.EvflowError(f"FlowStream: a sensor of {H} x {W} pixels (uint16 coordinates, int32 row offsets)")
        hf = config.get("hot_filter", {"enabled": False})
        self.hot = bool(hf.get("enabled", False))
        self._hot_params = (int(hf["max_px"]), int(hf["min_obvs"]), float(hf["max_rate"])) if self.hot else None
        self.window, self.slots, self.res, self.round_encoding = N, slots, (H, W), bool(round_encoding)
        self.num_bins = int(model.num_bins)
        self._want = ("cnt", "mask", "voxel") if model.encoding == "voxel" else ("cnt", "mask")
        self._t0_arg = self.t0 = None if t0 is None else float(t0)
        # ---- from here on the device
        if device is None:
            device = next(model.parameters()).device
        self.device = dev = torch.device(device)
        self.ring = EventRing(R, dev)
        self._init_replay(model, warmup, replay)
        self.table = StaticTable(_WindowTable(dev), TABLE_WORDS)
        self.ev = torch.empty((1, 1, N, 4), dtype=torch.float32, device=dev)
        self.dt_input = torch.empty((1, 1), dtype=torch.float64, device=dev)
        if self.hot:
            self._m = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
            self._hot_events = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
            self._hot_obvs = torch.zeros(1, dtype=torch.int32, device=dev)
        self.results = torch.zeros((slots, 3, H, W), dtype=torch.float32, device=dev)  # per row: flow [2,H,W], event mask [H,W]
        self._row_serial = [-1] * slots  # which window (counted over the stream's life) owns a row
        self.windows, self.pending, self._reset_next = 0, 0, True
        self.stats.update(windows=0, pushes=0, appends=0)

    # ------------------------------------------------------------------ the table and the launches
    def _capture(self):
        """`_ReplayedSteps._capture` with the cycle collector held off: an object it frees in the middle of a capture -- another
        stream's graphs, an event -- makes runtime calls that a capture in global mode does not allow."""
        was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            super()._capture()
        finally:
            if was:
                gc.enable()

    def _launches(self, reset):
        """The launches of one window on the static buffers -> what must stay allocated.  `reset` None: a captured graph, the
        state tensors are zero-filled under the table's reset word; else the eager `model.reset_states()`."""
        N, (H, W), ring = self.window, self.res, self.ring
        at = self.table.table_dev.data_ptr()
        _lib.call("evf_ring_cut", _lib.ptr(ring.xs), _lib.ptr(ring.ys), _lib.ptr(ring.ts), _lib.ptr(ring.ps), ring.capacity, at, at + 8,
                  at + 16, 1, 1, N, H, W, _lib.ptr(self.ev), _lib.ptr(self.dt_input))
        if self.hot:
            _lib.call("evf_hot_pixels", _lib.ptr(self.ev), at + 20, _lib.ptr(self._hot_events), _lib.ptr(self._hot_obvs),
                      _lib.ptr(self._m), None, 1, 1, N, H, W, *self._hot_params)
        d = encode_window(self.ev, self.num_bins, self.res, round_ts=self.round_encoding, want=self._want)[0]
        if self.hot:
            for key, C in (("event_voxel", self.num_bins), ("event_cnt", 2), ("event_mask", 1)):
                if key in d:
                    _lib.call("evf_apply_pixel_mask", _lib.ptr(d[key]), _lib.ptr(self._m), 1, C, H, W)
        if reset is None:
            zero_states_if(at + 24, self.model.state_buffers())
        elif reset:
            self.model.reset_states()
        self.model.mark_last_pass()  # (every window ends its graph: the next one starts from the state it leaves)
        x = self.model(d.get("event_voxel"), d["event_cnt"])
        flow = x["flow"][-1].detach().to(torch.float32).contiguous()
        mask = d["event_mask"].contiguous()
        HW = H * W
        _lib.call("evf_store_segments_at", at + 32, self.slots, _lib.ptr(self.results), 3 * HW,
                  (ctypes.c_void_p * 32)(_lib.ptr(flow), _lib.ptr(mask)), (ctypes.c_int * 32)(0, 2 * HW), (ctypes.c_int * 32)(2 * HW, HW), 2)
        return d, flow, mask

    # ------------------------------------------------------------------ the public calls
    @property
    def appended(self):
        return self.ring.appended

    @property
    def max_push(self):
        """The longest push accepted now."""
        return self.slots * self.window - self.pending

    def push(self, xs, ys, ts, ps):
        """Append the events, run every window that is complete -> its results, in order (possibly none)."""
        H, W = self.res
        x, y, t, p = check_events(xs, ys, ts, ps, H, W)
        ops = plan_push(self.pending, len(x), self.window, self.ring.capacity, self.slots, self.windows)
        if not ops:
            return []
        if self.t0 is None:
            self.t0 = float(t[0])
        t = t - self.t0
        out = []
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        for op in ops:
            if op[0] == "append":
                _, lo, hi = op
                with torch.cuda.stream(self.stream):
                    self.ring.append(x[lo:hi], y[lo:hi], t[lo:hi], p[lo:hi])
                self.pending += hi - lo
                self.stats["appends"] += 1
            else:
                out.append(self._window(*op[1:]))
        cur.wait_stream(self.stream)
        self.stats["pushes"] += 1
        return out

    def _window(self, k, first, row):
        N, R = self.window, self.ring.capacity
        job = (first, self.ring.appended, self._reset_next, row)
        reset, self._reset_next = self._reset_next, False

        def send():
            self.table.stage(job, self.seen)
            self.table.send()

        self._step(send, reset, reset)
        ready = torch.cuda.Event()
        ready.record(self.stream)
        self._row_serial[row] = serial = self.stats["windows"]
        self.stats["windows"] += 1
        self.windows, self.pending = k + 1, self.pending - N
        mirror = self.ring.ts_host
        return FlowResult(self, serial, row, k, first, float(mirror[first % R]), float(mirror[(first + N - 1) % R]), ready)

    def reset(self):
        """A new sequence: the next window zero-fills the recurrent state (the loop's `model.reset_states()`) and restarts the
        hot-pixel statistics; pending events are dropped; the stream index and t0 start again.  Results handed out stay valid
        until their rows are reused."""
        self._reset_next = True
        self.windows = self.pending = 0
        self.t0 = self._t0_arg
        self.ring.restart()

    def synchronize(self):
        """Wait for everything pushed so far (a host wait; `push` itself never does this)."""
        self.stream.synchronize()
