"""Rig streaming: optical flow at a fixed rate from the pushed events of B synchronised cameras.  `RigStream.push(events)` takes one
`(xs, ys, ts, ps)` tuple per camera, appends all of them to B device rings (the columns of `stream.EventRing` as [B, R];
csrc/evf_stream.hip) with ONE pinned -> device copy and ONE launch (evf_rings_append), and runs every window of `window_dt` seconds
that every camera has passed: window k of every camera is the same interval, so the B windows are one batch -- one copy of one
table and, behind the warm-up, one launch of two alternately replayed graphs (evaluate._ReplayedSteps) holding the cut
(evf_rings_cut_ragged: evf_seq_cut_ragged's rows bit for bit), the hot-pixel filter, the binning, the mask launches, the conditional
zero-fill of the recurrent state, the forward under no_grad and the store of flow and event mask into a ring of `slots` result rows.

What the host decides needs no device value: it sees every pushed timestamp (`check_events` reads them), so `plan_tick` -- a pure
function -- names every window's first event and event count per camera before the launch.

Borders are the reference loader's cursor in `data.mode: time` (dataloader/h5.py:232-264, mirrored in `ResidentEvalPlan`): `row`
starts at 0 and advances by `row += dt` in float64 (never k * dt); window k holds the events with row_k + t0 <= ts < (row_k + t0) +
dt, compared on the ABSOLUTE float64 timestamps as pushed; the index of a border is the LEFTMOST event with ts >= border.  That is
`binary_search_array` whenever the timestamps around a border are distinct.  The one difference: with several equal timestamps
exactly on a border the reference returns whichever of them its bisection meets first, which depends on the length of the file; a
stream cannot know that length, so it takes the leftmost.  Nor does a stream know where a file ends: the loader's rule that the
window holding a file's last event starts the next file has no counterpart here.  A window with at most 10 events in a camera is cut
as empty for that camera (count = 0; h5.py:268); the forward still runs.

Watermarks: camera b has passed time T when it has pushed an event with ts >= T, or when the caller declared it with `advance(t)`,
t >= T ("every camera has delivered everything before t"); a window runs when every camera has passed its closing border.  The
declaration is what keeps an idle camera from stalling the rig.

Fused FireNets only, one process: `stream.stream_refusal`.  `cameras=1` is the single-camera time-window stream."""

import ctypes
import gc

import numpy as np
import torch

from . import _lib
from .dataloader.encodings import encode_window
from .dataloader.resident import StaticTable, zero_states_if
from .evaluate import _ReplayedSteps
from .stream import CHUNK_RING, check_events, stream_refusal

MAX_CAMERAS = 16   # evf_rings_append walks at most 17 offsets a thread; 2 * 16 segments fill one evf_store_segments_at
EMPTY_UP_TO = 10   # a window of up to 10 events is an empty window (dataloader/h5.py:268)


def table_words(B):
    """int64 words of a tick's table: first [B] | appended [B] | as int32: count [B], flags [B], hot-pixel reset [B], state reset,
    pad to a whole word | the result row."""
    return 2 * B + (3 * B + 2) // 2 + 1


def window_borders(row, t0, dt):
    """(opening, closing) border of the window at cursor `row`, absolute float64: the loader's (row + t0, (row + t0) + window)."""
    begin = float(row) + float(t0)
    return begin, begin + float(dt)


def border_index(ts, border):
    """Index of a border in ascending timestamps: the leftmost event with ts >= border (see the module for the one difference
    from `binary_search_array`)."""
    return int(np.searchsorted(ts, border, side="left"))


def plan_tick(pending, base, passed, row, t0, dt, max_events, overflow="raise"):
    """The window at cursor `row`, decided on the host.  pending[b]: the absolute float64 timestamps, ascending, of camera b's
    events from stream index base[b] on (everything not behind an earlier window); passed[b]: the time camera b has passed.
    -> None while some camera has not passed the closing border, else (jobs, next row), jobs[b] = (first, count, dropped, done):
    the window holds `count` events from camera b's stream index `first` on, `dropped` older ones of the window were left out
    (`overflow="newest"`: the newest `max_events` stay; "raise": EvflowError), and the first `done` entries of pending[b] lie
    before the next window's opening border."""
    begin, end = window_borders(row, t0, dt)
    if not end > begin:
        raise _lib.EvflowError(f"a window_dt of {dt!r} s does not advance a cursor at {begin!r} s")
    if any(not p >= end for p in passed):
        return None
    nxt = float(row) + float(dt)
    jobs = []
    for b, (ts, at) in enumerate(zip(pending, base)):
        lo, hi = border_index(ts, begin), border_index(ts, end)
        first, n, dropped = int(at) + lo, hi - lo, 0
        if n > max_events:
            if overflow != "newest":
                raise _lib.EvflowError(f"camera {b}: the window [{begin!r}, {end!r}) holds {n} events, more than max_events = "
                                       f"{max_events}: build the stream with a larger max_events or a shorter window_dt, or with "
                                       "overflow='newest' to keep the newest events of such a window")
            dropped = n - max_events
            first, n = first + dropped, max_events
        jobs.append((first, n if n > EMPTY_UP_TO else 0, dropped, max(border_index(ts, nxt + float(t0)), lo)))
    return jobs, nxt


class RigPlan:
    """The host-only half of `RigStream` (no GPU): per camera the events appended, the timestamps that are not behind a window yet
    and the watermark; the cursor `row` and the window number.  `plan(...)` decides a whole call -- the append and every window it
    completes -- on copies and raises every refusal there; `commit` makes it the state."""

    def __init__(self, cameras, window_dt, max_events, capacity=None, slots=8, t0=None, overflow="raise"):
        B, Npad, slots = int(cameras), int(max_events), int(slots)
        R = 4 * Npad if capacity is None else int(capacity)
        dt = float(window_dt)
        if not 1 <= B <= MAX_CAMERAS:
            raise _lib.EvflowError(f"RigStream: {cameras} cameras (1 .. {MAX_CAMERAS})")
        if not (dt > 0 and np.isfinite(dt)) or Npad < 1 or slots < 1 or R < Npad:
            raise _lib.EvflowError(f"RigStream: windows of {window_dt!r} s (> 0) with up to {Npad} events (at least 1) in rings of {R} "
                                   f"slots (at least max_events) with {slots} result rows (at least 1)")
        if overflow not in ("raise", "newest"):
            raise _lib.EvflowError(f"RigStream: overflow={overflow!r} ('raise' or 'newest')")
        self.cameras, self.window_dt, self.max_events, self.capacity, self.slots, self.overflow = B, dt, Npad, R, slots, overflow
        self._t0_arg = None if t0 is None else float(t0)
        self.restart()

    def restart(self):
        B = self.cameras
        self.t0, self.row, self.windows, self.declared = self._t0_arg, 0.0, 0, -np.inf
        self.appended, self.base = [0] * B, [0] * B
        self.pending = [np.zeros(0, dtype=np.float64) for _ in range(B)]
        self.last = [-np.inf] * B

    def counters(self):
        """Everything a refused call must leave as it was."""
        return (self.t0, self.row, self.windows, self.declared, tuple(self.appended), tuple(self.base),
                tuple(len(p) for p in self.pending), tuple(self.last))

    @property
    def uncut(self):
        """Per camera: events in its ring that no window is behind yet."""
        return [len(p) for p in self.pending]

    def plan(self, ts=None, advance=None):
        """A call decided on copies: `ts` one ascending float64 array of absolute timestamps per camera (a push), and / or
        `advance` a declared watermark -> (state, heads, ticks): the state to `commit`, per camera the stream index its pushed
        events start at, and per completed window (index, row, jobs of `plan_tick`, appended per camera, result row)."""
        B, R = self.cameras, self.capacity
        t0, row, windows, declared = self.t0, self.row, self.windows, self.declared
        appended, base, pending, last = list(self.appended), list(self.base), list(self.pending), list(self.last)
        heads = list(appended)
        if ts is not None:
            if len(ts) != B:
                raise _lib.EvflowError(f"push: one (xs, ys, ts, ps) tuple per camera, got {len(ts)} for {B} cameras")
            for b, t in enumerate(ts):
                if len(t) and (t[0] < last[b] or np.any(t[1:] < t[:-1])):
                    raise _lib.EvflowError(f"push: camera {b}'s timestamps go backwards (its last one was {last[b]!r}): push every "
                                           "camera's events in time order, or reset() the stream for a new recording")
            if t0 is None and any(len(t) for t in ts):
                t0 = min(float(t[0]) for t in ts if len(t))
            for b, t in enumerate(ts):
                if not len(t):
                    continue
                if len(pending[b]) + len(t) > R:
                    passed = [max(l, declared) for l in last]
                    lag = int(np.argmin(passed))
                    end = window_borders(row, t0, self.window_dt)[1]
                    raise _lib.EvflowError(
                        f"push: {len(t)} events for camera {b} would overwrite events of its ring ({R} slots, {len(pending[b])} not "
                        f"cut yet) that window {windows} still needs; the window waits for camera {lag}, which has only passed "
                        f"{passed[lag]!r} of its closing border {end!r}: push camera {lag}'s events first, or advance(t) past the "
                        f"border, or push at most {R - len(pending[b])} events, or build the stream with a larger capacity")
                pending[b] = np.concatenate([pending[b], t])
                appended[b] += len(t)
                last[b] = float(t[-1])
        if advance is not None:
            if not np.isfinite(advance):
                raise _lib.EvflowError(f"advance: a watermark of {advance!r}")
            declared = max(declared, float(advance))
        ticks = []
        if t0 is not None:
            passed = [max(l, declared) for l in last]
            while True:
                tick = plan_tick(pending, base, passed, row, t0, self.window_dt, self.max_events, self.overflow)
                if tick is None:
                    break
                if len(ticks) == self.slots:
                    raise _lib.EvflowError(f"this call completes more than {self.slots} windows of {self.window_dt!r} s, whose results "
                                           f"would overwrite each other in the {self.slots} result rows: push or advance in smaller "
                                           "steps, or build the stream with more slots")
                jobs, nxt = tick
                ticks.append((windows, row, [j[:3] for j in jobs], list(appended), windows % self.slots))
                for b, j in enumerate(jobs):
                    pending[b], base[b] = pending[b][j[3]:], base[b] + j[3]
                row, windows = nxt, windows + 1
        return (t0, row, windows, declared, appended, base, pending, last), heads, ticks

    def commit(self, state):
        self.t0, self.row, self.windows, self.declared, self.appended, self.base, self.pending, self.last = state


class RigRings:
    """The device rings of a rig: the four columns of `stream.EventRing` as [B, R], ring b at offset b R, camera b's stream event e
    at slot e mod R; a staging buffer in device memory (int64 head [B] | int64 offsets [B + 1] | the chunk ts | xs | ys | ps of
    all cameras in camera order) with a ring of pinned host copies, each with an event recorded after its copy."""

    def __init__(self, cameras, capacity, device):
        self.cameras, self.capacity = B, R = int(cameras), int(capacity)
        _lib.load()
        if not torch.cuda.is_available() or torch.device(device).type != "cuda":
            raise _lib.EvflowError("RigRings: the events live and are cut on the MI355X only (no CPU fallback)")
        self.device = dev = torch.device(device)
        self.xs = torch.zeros((B, R), dtype=torch.int16, device=dev)  # (uint16 bits)
        self.ys = torch.zeros((B, R), dtype=torch.int16, device=dev)
        self.ts = torch.zeros((B, R), dtype=torch.float64, device=dev)
        self.ps = torch.zeros((B, R), dtype=torch.uint8, device=dev)
        size = 8 * (2 * B + 1) + 13 * B * R
        self.stage_dev = torch.empty(size, dtype=torch.uint8, device=dev)
        self.chunks = [(torch.empty(size, dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(CHUNK_RING)]
        self.copies = 0

    def append(self, heads, cols):
        """One push: cols[b] = (xs uint16, ys uint16, ts float64, ps uint8) of camera b (at most `capacity` each, possibly none),
        heads[b] its stream index -> one pinned -> device copy of the staged buffer, one evf_rings_append."""
        B, R = self.cameras, self.capacity
        counts = [len(c[0]) for c in cols]
        n, most = sum(counts), max(counts)
        if most > R:
            raise _lib.EvflowError(f"RigRings.append: {most} events into a ring of {R}")
        if n == 0:
            return
        pinned, copied = self.chunks[self.copies % CHUNK_RING]
        copied.synchronize()  # (the copy that read this pinned chunk CHUNK_RING appends ago)
        host = pinned.numpy()
        words = host[:8 * (2 * B + 1)].view(np.int64)
        words[:B] = heads
        words[B] = 0
        words[B + 1:] = np.cumsum(counts)
        at = 8 * (2 * B + 1)
        for k, (dtype, size) in enumerate(((np.float64, 8), (np.uint16, 2), (np.uint16, 2), (np.uint8, 1))):
            col = host[at:at + size * n].view(dtype)
            lo = 0
            for c, m in zip(cols, counts):
                col[lo:lo + m] = c[(2, 0, 1, 3)[k]]
                lo += m
            at += size * n
        self.stage_dev[:at].copy_(pinned[:at], non_blocking=True)
        copied.record()
        _lib.call("evf_rings_append", self.stage_dev.data_ptr(), B, n, most, _lib.ptr(self.xs), _lib.ptr(self.ys), _lib.ptr(self.ts),
                  _lib.ptr(self.ps), R)
        self.copies += 1


class RigResult:
    """One window's result for all cameras.  `index`: the window's number since the last reset, `t_begin` / `t_end`: its borders
    relative to the stream's t0; per camera `first` (stream index of its first event), `count` (0: an empty window) and `dropped`
    (overflow="newest"); `ready`: an event recorded behind the window's launches.  `flow` [B,2,H,W], `event_mask` [B,H,W] and
    `flow_masked` are VIEWS into the stream's result ring, ordered behind the window on the stream the call was made on; once
    `slots` later windows have run the row is reused, and the access raises."""

    def __init__(self, stream, serial, row, index, t_begin, t_end, jobs, ready):
        self._stream, self._serial, self._row = stream, serial, row
        self.index, self.t_begin, self.t_end, self.ready = index, t_begin, t_end, ready
        self.first, self.count, self.dropped = ([j[k] for j in jobs] for k in range(3))

    def _view(self):
        if self._stream._row_serial[self._row] != self._serial:
            raise _lib.EvflowError(f"RigResult: window {self.index}'s row {self._row} of the result ring has been reused by a later "
                                   f"window (the ring holds the last {self._stream.slots} results): copy a result before that many "
                                   "later windows run, or build the stream with more slots")
        return self._stream.results[self._row]

    @property
    def flow(self):
        return self._view()[:, :2]

    @property
    def event_mask(self):
        return self._view()[:, 2]

    @property
    def flow_masked(self):
        """eval_flow.py's `flow_vis`: the flow times the event mask when the model masks its output, else the flow."""
        row = self._view()
        return row[:, :2] * row[:, 2:3] if self._stream.model.mask else row[:, :2]


class _TickTable:
    """What `StaticTable` asks of a loader, for one window of B cameras a step (an object of its own, like stream._WindowTable, so
    that the stream and its table do not refer to each other)."""

    def __init__(self, device, cameras):
        self.device, self.cameras = device, cameras

    def _job_table(self, job):
        """The words of one tick (see `table_words`); no flips on a live stream."""
        jobs, appended, reset, row = job
        B = self.cameras
        tab = np.zeros(table_words(B), dtype=np.int64)
        tab[:B] = [j[0] for j in jobs]
        tab[B:2 * B] = appended
        aux = tab[2 * B:-1].view(np.int32)
        aux[:B] = [j[1] for j in jobs]
        aux[2 * B:3 * B + 1] = 1 if reset else 0
        tab[-1] = row
        return tab


class RigStream(_ReplayedSteps):
    """Flow from the pushed events of `cameras` synchronised cameras, one result every `window_dt` seconds (see the module).

        rig = RigStream(model, config, cameras=2, window_dt=0.01, max_events=30000)   # config: loader.resolution, hot_filter
        for left, right in source:                          # one (xs, ys, ts, ps) tuple of host arrays per camera, any may be empty
            for r in rig.push([left, right]):
                use(r.flow)                                 # [B,2,H,W] device views; r.ready.synchronize() before a host read
        rig.advance(t)                                      # every camera has delivered everything before t

    `max_events`: the padded width of a window (`overflow` decides about a fuller one); `capacity`: slots of every camera's event
    ring (default 4 max_events); `slots`: rows of the result ring; `t0`: the stream's time origin (default: the earliest timestamp
    of the first push), subtracted from every timestamp in float64; the first `warmup` (>= 2) windows and every window with
    `replay=False` run the launches eagerly.  Neither call reads a device value or synchronises the device."""

    def __init__(self, model, config, cameras, window_dt, max_events, capacity=None, slots=8, t0=None, overflow="raise", warmup=2,
                 replay=True, round_encoding=False, device=None):
        why = stream_refusal(model)
        if why:
            raise _lib.EvflowError(why.replace("FlowStream", "RigStream"))
        self.plan = plan = RigPlan(cameras, window_dt, max_events, capacity, slots, t0, overflow)
        B, Npad = plan.cameras, plan.max_events
        H, W = (int(v) for v in config["loader"]["resolution"])
        if H < 1 or W < 1 or H > 65535 or W > 65535 or 3 * B * H * W >= 2 ** 31:
            raise _lib.EvflowError(f"RigStream: {B} sensors of {H} x {W} pixels (uint16 coordinates, int32 row offsets)")
        hf = config.get("hot_filter", {"enabled": False})
        self.hot = bool(hf.get("enabled", False))
        self._hot_params = (int(hf["max_px"]), int(hf["min_obvs"]), float(hf["max_rate"])) if self.hot else None
        self.cameras, self.max_events, self.slots, self.res, self.round_encoding = B, Npad, plan.slots, (H, W), bool(round_encoding)
        self.num_bins = int(model.num_bins)
        self._want = ("cnt", "mask", "voxel") if model.encoding == "voxel" else ("cnt", "mask")
        # ---- from here on the device
        if device is None:
            device = next(model.parameters()).device
        self.device = dev = torch.device(device)
        self.rings = RigRings(B, plan.capacity, dev)
        self._init_replay(model, warmup, replay)
        self.table = StaticTable(_TickTable(dev, B), table_words(B))
        self.ev = torch.empty((B, 1, Npad, 4), dtype=torch.float32, device=dev)
        self.dt_input = torch.empty(B, dtype=torch.float64, device=dev)
        if self.hot:
            self._m = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
            self._hot_events = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
            self._hot_obvs = torch.zeros(B, dtype=torch.int32, device=dev)
        self.results = torch.zeros((plan.slots, B, 3, H, W), dtype=torch.float32, device=dev)  # per camera: flow [2,H,W], mask [H,W]
        self._row_serial = [-1] * plan.slots  # which window (counted over the stream's life) owns a row
        self._reset_next = True
        self.stats.update(windows=0, pushes=0, appends=0)

    # ------------------------------------------------------------------ the table and the launches
    def _capture(self):
        """`_ReplayedSteps._capture` with the cycle collector held off (see stream.FlowStream._capture)."""
        was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            super()._capture()
        finally:
            if was:
                gc.enable()

    def _launches(self, reset):
        """The launches of one tick on the static buffers -> what must stay allocated.  `reset` None: a captured graph, the state
        tensors are zero-filled under the table's reset word; else the eager `model.reset_states()`."""
        B, Npad, (H, W), rings = self.cameras, self.max_events, self.res, self.rings
        at = self.table.table_dev.data_ptr()
        aux = at + 16 * B  # int32: count [B] | flags [B] | hot-pixel reset [B] | state reset
        _lib.call("evf_rings_cut_ragged", _lib.ptr(rings.xs), _lib.ptr(rings.ys), _lib.ptr(rings.ts), _lib.ptr(rings.ps), rings.capacity,
                  at, at + 8 * B, aux, aux + 4 * B, B, Npad, H, W, _lib.ptr(self.ev), _lib.ptr(self.dt_input))
        if self.hot:  # (an empty window is an observation too, like create_hot_mask's)
            _lib.call("evf_hot_pixels", _lib.ptr(self.ev), aux + 8 * B, _lib.ptr(self._hot_events), _lib.ptr(self._hot_obvs),
                      _lib.ptr(self._m), None, B, 1, Npad, H, W, *self._hot_params)
        d = encode_window(self.ev, self.num_bins, self.res, round_ts=self.round_encoding, want=self._want)[0]
        if self.hot:
            for key, C in (("event_voxel", self.num_bins), ("event_cnt", 2), ("event_mask", 1)):
                if key in d:
                    _lib.call("evf_apply_pixel_mask", _lib.ptr(d[key]), _lib.ptr(self._m), B, C, H, W)
        if reset is None:
            zero_states_if(aux + 12 * B, self.model.state_buffers())
        elif reset:
            self.model.reset_states()
        self.model.mark_last_pass()  # (every window ends its graph: the next one starts from the state it leaves)
        x = self.model(d.get("event_voxel"), d["event_cnt"])
        flow = x["flow"][-1].detach().to(torch.float32).contiguous()
        mask = d["event_mask"].contiguous()
        HW = H * W
        src = [t.data_ptr() + 4 * b * k * HW for b in range(B) for t, k in ((flow, 2), (mask, 1))]
        off = [3 * b * HW + o for b in range(B) for o in (0, 2 * HW)]
        cnt = [2 * HW, HW] * B
        _lib.call("evf_store_segments_at", at + 8 * (table_words(B) - 1), self.slots, _lib.ptr(self.results), 3 * B * HW,
                  (ctypes.c_void_p * 32)(*src), (ctypes.c_int * 32)(*off), (ctypes.c_int * 32)(*cnt), 2 * B)
        return d, flow, mask

    # ------------------------------------------------------------------ the public calls
    @property
    def appended(self):
        """Per camera: events pushed since the last reset."""
        return list(self.plan.appended)

    @property
    def max_push(self):
        """Per camera: the longest push its ring accepts now."""
        return [self.plan.capacity - n for n in self.plan.uncut]

    @property
    def t0(self):
        return self.plan.t0

    def push(self, events):
        """Append one `(xs, ys, ts, ps)` tuple per camera (any may be empty), run every window that is complete -> the results, in
        order (possibly none)."""
        H, W = self.res
        if len(events) != self.cameras:
            raise _lib.EvflowError(f"push: one (xs, ys, ts, ps) tuple per camera, got {len(events)} for {self.cameras} cameras")
        cols = [check_events(*e, H, W) for e in events]
        state, heads, ticks = self.plan.plan(ts=[c[2] for c in cols])
        return self._run(state, heads, cols, ticks)

    def advance(self, t):
        """Declare that every camera has delivered everything before the absolute time `t` -> the results of the windows this
        completes, in order."""
        state, heads, ticks = self.plan.plan(advance=float(t))
        return self._run(state, heads, None, ticks)

    def _run(self, state, heads, cols, ticks):
        t0 = state[0]
        self.plan.commit(state)
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        if cols is not None and any(len(c[0]) for c in cols):
            with torch.cuda.stream(self.stream):
                self.rings.append(heads, [(x, y, t - t0, p) for x, y, t, p in cols])
            self.stats["appends"] += 1
        out = [self._tick(*tick) for tick in ticks]
        cur.wait_stream(self.stream)
        if cols is not None:
            self.stats["pushes"] += 1
        return out

    def _tick(self, k, row, jobs, appended, res_row):
        job = (jobs, appended, self._reset_next, res_row)
        reset, self._reset_next = self._reset_next, False

        def send():
            self.table.stage(job, self.seen)
            self.table.send()

        self._step(send, reset, reset)
        ready = torch.cuda.Event()
        ready.record(self.stream)
        self._row_serial[res_row] = serial = self.stats["windows"]
        self.stats["windows"] += 1
        return RigResult(self, serial, res_row, k, row, row + self.plan.window_dt, jobs, ready)

    def reset(self):
        """A new recording on all cameras together: the next window zero-fills the recurrent state and restarts the hot-pixel
        statistics; events not behind a window are dropped; stream indices, the cursor and t0 start again.  Results handed out stay
        valid until their rows are reused."""
        self._reset_next = True
        self.plan.restart()

    def synchronize(self):
        """Wait for everything pushed so far (a host wait; `push` and `advance` never do this)."""
        self.stream.synchronize()
