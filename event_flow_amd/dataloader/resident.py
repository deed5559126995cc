"""Device-resident event sequences: every sequence file of the loader's shard is uploaded ONCE, and every batch -- or every
whole BPTT window -- is then cut, formatted, flipped, filtered and binned by kernels (csrc/evf_resident.hip + the existing
binning), with the keys, shapes, dtypes and values `H5Loader` gives on the same files, flags and RNG state.  The cursor, the column reader and the arena are shared with the
evaluation loader: dataloader/resident_base.py.

Only `data.mode: events` (the training mode): there the next window of a slot is index arithmetic on the sequence LENGTHS,
so the host decides everything without a device value.  That decision is `ResidentPlan` -- `ResidentCursor` plus the cursor
step of dataloader/h5.py:244-279,310 written over lengths.  It needs no GPU.  `ResidentLoader` adds the arena and the launches,
`ResidentWindow` the static buffers of a window that is cut again and again (the graph-replayed steppers), over `StaticTable`,
the job table at a fixed device address with its ring of pinned host copies (shared with the evaluation loader's window).

Layout in device memory: one arena per column over all files, `xs`, `ys` uint16, `ts` float64 RELATIVE to its file's t0
(subtracted on the host in float64 exactly like `get_events`), `ps` uint8 -- 13 bytes per event -- and int64 offsets."""

import ctypes

import numpy as np
import torch

from .. import _lib
from .encodings import encode_event_list, encode_window
from .h5 import open_sequence
from .resident_base import FLAG_BITS, ResidentArena, ResidentCursor, read_columns  # noqa: F401  (FLAG_BITS: imported from here)


class ResidentPlan(ResidentCursor):
    """The host-only half: which (sequence file, first event, flip flags) every slot reads next, and whether the slot
    restarted on the way -- the same decisions, counters and `np.random.random()` draws, in the same order, as
    `H5Loader.__getitem__` in `events` mode.  `lengths`: events per file (path -> int); read from the files when omitted."""

    def __init__(self, config, num_bins, round_encoding=False, device=None, rank=0, world_size=1, lengths=None):
        mode, window = config["data"]["mode"], config["data"]["window"]
        if mode != "events":
            raise _lib.EvflowError(f"ResidentLoader serves data.mode 'events' only, not '{mode}' (windows by time, frame or "
                                   "ground-truth map need a search per window and give ragged batches): use H5Loader")
        if isinstance(window, bool) or int(window) != window or window <= 10:
            raise _lib.EvflowError(f"ResidentLoader needs an integer data.window > 10, got {window!r} (the reference hands "
                                   "windows of up to 10 events on as empty ones, dataloader/h5.py:268): use H5Loader")
        self._slot_path = {}
        super().__init__(config, num_bins, round_encoding, device, prefetch=0, rank=rank, world_size=world_size)
        self.window = int(window)
        self.lengths = dict(lengths) if lengths is not None else self._read_lengths()
        if max(self.lengths[f] for f in self.files) < self.window:
            raise _lib.EvflowError(f"no sequence file holds one window of {self.window} events")
        self._stream = None

    def _read_lengths(self):
        out = {}
        for path in self.files:
            seq = open_sequence(path)
            out[path] = len(seq.events("xs"))
            seq.close()
        return out

    def plan_sample(self, batch):
        """dataloader/h5.py:244-279,310 for one slot -> (path, first event, flags, restarted)."""
        restarted = False
        while self.lengths[self._slot_path[batch]] - self.batch_row[batch] < self.window:  # fewer events left than a window
            restarted = True
            self._restart(batch)
        first = self.batch_row[batch]
        self.batch_row[batch] += self.window
        return self._slot_path[batch], first, self.slot_flags(batch), restarted

    def _endless(self):
        """The batches of pass after pass over the files, as the training driver meets them: (jobs, restarted, done)."""
        while True:
            for jobs, (restarted, done) in self.plan_batches():
                self._delivered(restarted, done)
                yield jobs, restarted, done
            self._end_pass()

    def plan_window(self, P):
        """The next group of P consecutive batches on which train_flow.py's loop takes an optimizer step (threshold
        window_loss = P * window) -> (discarded, group, reset).  `discarded`: the batches the loop forwarded before
        and then dropped because a later batch restarted a slot; `reset`: the loop reset model, loss and gradients in
        front of the group's first batch.  A partial group survives the end of a pass over the files, as in the loop."""
        if self._stream is None:
            self._stream = self._endless()
        discarded, group, reset = [], [], False
        while len(group) < P:
            jobs, restarted, done = next(self._stream)
            if restarted:  # train_flow.py:92-96: everything collected so far is dropped
                discarded += group
                group, reset = [], True
            group.append((jobs, restarted, done))
        return discarded, group, reset

    def plan_steps(self, P, n_epochs):
        """The optimizer steps of `n_epochs` passes over the files, as train_flow.py's loop takes them: (discarded, group,
        reset, epoch) per step, `plan_window`'s triple and the pass the step belongs to.  A batch belongs to pass e when e
        wrap-around (`done`) batches were delivered strictly before it, a step to the pass of its group's last batch; the
        generator ends before the first step whose last batch lies in pass `n_epochs` (a partial group at the end is not
        stepped)."""
        wraps = 0  # `done` batches delivered so far
        while True:
            discarded, group, reset = self.plan_window(P)
            epoch = wraps + sum(1 for _j, _r, done in discarded + group[:-1] if done)
            if epoch >= n_epochs:
                return
            yield discarded, group, reset, epoch
            wraps = epoch + (1 if group[-1][2] else 0)

    def plan_eval_steps(self, P):
        """ONE pass over the files as eval_flow.py's loop meets it: the batches of `plan_batches()` up to, not including, the
        wrap-around (`done`) batch -- the loop breaks on that one before forwarding it -- in groups of P consecutive batches:
        (group, pass_reset, tail) per group, `group` P batches (jobs, restarted, done) like `plan_window`'s, `pass_reset[p]`
        whether batch p restarted a slot (the loop's `model.reset_states()` in front of that pass), `tail` False; at the end
        once (rest, its pass_reset, True) with the fewer than P batches left over (possibly none).  The loop does not reset
        its criteria at a new sequence and every batch adds `window` events, so a criterion fires after every P =
        ceil(window_eval / window) batches whatever restarts: the groups are the metric windows.  Independent of
        `plan_window` / `plan_steps` (it does not touch their stream); the loader's flags, sample counter and end-of-pass
        bookkeeping move as in `__iter__`."""
        P = int(P)
        if P < 1:
            raise _lib.EvflowError(f"plan_eval_steps: groups of {P} batches")
        group = []
        try:
            for jobs, (restarted, done) in self.plan_batches():
                self._delivered(restarted, done)
                if done:
                    break
                group.append((jobs, restarted, done))
                if len(group) == P:
                    yield group, [r for _j, r, _d in group], False
                    group = []
            yield group, [r for _j, r, _d in group], True
        finally:
            self._end_pass()


class ResidentLoader(ResidentArena, ResidentPlan):
    def __init__(self, config, num_bins, round_encoding=False, device=None, rank=0, world_size=1):
        super().__init__(config, num_bins, round_encoding, device, rank, world_size)  # (reads the columns: _read_lengths)
        cols, self._cols = self._cols, None
        _lib.load()  # the refusals above are host work; from here on the device
        if not torch.cuda.is_available():
            raise _lib.EvflowError("ResidentLoader: the sequences live and are cut on the MI355X only (no CPU fallback)")
        self._place(self.lengths)
        self._upload(cols)

    def _read_lengths(self):
        """Every file's four columns, once (kept in self._cols until they are uploaded) -> their lengths."""
        self._cols, lengths = ([], [], [], []), {}
        for path in self.files:
            seq = open_sequence(path)
            for col, c in zip(self._cols, read_columns(seq, path)):  # (the absolute timestamps are not kept)
                col.append(c)
            seq.close()
            lengths[path] = len(self._cols[0][-1])
        return lengths

    # ------------------------------------------------------------------ launches
    def _job_table(self, batches):
        """The host table of P planned batches, job j = b * P + p: `first` int64 [B*P], then as int32 `flags` [B*P] | slot
        `reset` [B*P] | the window's `reset` (did the first batch restart a slot: train_flow.py's loop reset the model in front
        of it) -- one int64 array of 2*B*P + 1 words."""
        B, P = self.batch_size, len(batches)
        tab = np.zeros(2 * B * P + 1, dtype=np.int64)
        aux = tab[B * P:].view(np.int32)
        for p, (jobs, _restarted, _done) in enumerate(batches):
            for b, (path, first, flags, restarted) in enumerate(jobs):
                tab[b * P + p] = self.offsets[path] + first
                aux[b * P + p] = flags
                aux[B * P + b * P + p] = 1 if restarted else 0
        aux[2 * B * P] = 1 if batches[0][1] else 0
        self.last_row = (path, first + self.window - 1)  # last event of the last slot's last pass
        return tab

    def _buffers(self, P):
        """The buffers of a window of P batches: ev [B,P,N,4], dt_input [P,B] float64 and, with the hot filter, the masks m_bp
        [B,P,H,W] and m_pb [P,B,H,W] (None when P = 1: the same layout)."""
        B, N, dev = self.batch_size, self.window, self.device
        H, W = self.res
        ev = torch.empty((B, P, N, 4), dtype=torch.float32, device=dev)
        dt = torch.empty((P, B), dtype=torch.float64, device=dev)
        m_bp = torch.empty((B, P, H, W), dtype=torch.float32, device=dev) if self.hot else None
        m_pb = torch.empty((P, B, H, W), dtype=torch.float32, device=dev) if self.hot and P > 1 else None
        return ev, dt, m_bp, m_pb

    def _launch_cut(self, table_dev, P, ev, dt, m_bp=None, m_pb=None):
        """evf_seq_cut and, with the hot filter, evf_hot_pixels on a job table in device memory (`_job_table`'s layout), into
        the caller's `_buffers(P)`.  No allocation and no host copy: the launches can be captured."""
        B, N = self.batch_size, self.window
        H, W = self.res
        at = table_dev.data_ptr()
        _lib.call("evf_seq_cut", _lib.ptr(self._xs), _lib.ptr(self._ys), _lib.ptr(self._ts), _lib.ptr(self._ps), self.total_events,
                  at, at + 8 * B * P, B, P, N, H, W, _lib.ptr(ev), _lib.ptr(dt))
        if self.hot:
            _lib.call("evf_hot_pixels", _lib.ptr(ev), at + 12 * B * P, _lib.ptr(self._hot_events), _lib.ptr(self._hot_obvs),
                      _lib.ptr(m_bp), _lib.ptr(m_pb), B, P, N, H, W, *self._hot_params())

    def _cut(self, batches):
        """P planned batches -> fresh `_buffers(P)`, filled: one copy of the job table, one evf_seq_cut, one evf_hot_pixels."""
        t = torch.from_numpy(self._job_table(batches))
        t = t.pin_memory().to(self.device, non_blocking=True)
        buf = self._buffers(len(batches))
        self._launch_cut(t, len(batches), *buf)
        return buf

    def _window_passes(self, ev, dt, m_bp, m_pb, dt_gt=None):
        """Filled `_buffers(P)` -> the P batch dicts: the binning (`encode_window`), the hot-pixel masks applied in place to the
        window buffers, dt_input and dt_gt (rows of `dt_gt` [P,B]; zeros allocated here when None)."""
        B, P = self.batch_size, ev.shape[1]
        H, W = self.res
        passes = encode_window(ev, self.num_bins, self.res, round_ts=self.round_encoding)
        if self.hot:
            m_pb = m_pb if m_pb is not None else m_bp.view(P, B, H, W)
            # network inputs are pass-major ([P,B,C,H,W], one tensor per pass), the loss's mask stack batch-major ([B,P,H,W])
            cnt = torch.as_strided(passes[0]["event_cnt"], (P * B, 2, H, W), passes[0]["event_cnt"].stride())
            vox = torch.as_strided(passes[0]["event_voxel"], (P * B, self.num_bins, H, W), passes[0]["event_voxel"].stride())
            emask = torch.as_strided(passes[0]["event_mask"], (B * P, 1, H, W), (H * W, H * W, W, 1))
            _lib.call("evf_apply_pixel_mask", _lib.ptr(vox), _lib.ptr(m_pb), P * B, self.num_bins, H, W)
            _lib.call("evf_apply_pixel_mask", _lib.ptr(cnt), _lib.ptr(m_pb), P * B, 2, H, W)
            _lib.call("evf_apply_pixel_mask", _lib.ptr(emask), _lib.ptr(m_bp), B * P, 1, H, W)
        if dt_gt is None:
            dt_gt = torch.zeros((P, B), dtype=torch.float64, device=self.device)
        for p, d in enumerate(passes):
            d["dt_gt"], d["dt_input"] = dt_gt[p], dt[p]
        return passes

    def window_passes(self, batches):
        """P planned batches -> their batch dicts, cut by ONE launch into one fresh [B,P,N,4] buffer: the allocating twin of
        `ResidentWindow.launch`."""
        return self._window_passes(*self._cut(batches))

    def _produce(self, jobs, restarted, done):
        """One planned batch -> the reference's batch dict (dataloader/base.py:248-265)."""
        B = self.batch_size
        ev, dt, m_bp, _m_pb = self._cut([(jobs, restarted, done)])
        out = encode_event_list(ev.view(B, self.window, 4), self.num_bins, self.res, round_ts=self.round_encoding)
        if self.hot:
            self._mask_batch(out, m_bp)
        out["dt_gt"] = torch.zeros(B, dtype=torch.float64, device=self.device)
        out["dt_input"] = dt[0]
        return out

    def next_window(self, P):
        """-> (passes, reset): the P batch dicts of the next group of batches on which train_flow.py's loop steps the
        optimizer (see `plan_window`), cut by ONE launch into one [B,P,N,4] buffer and binned by `encode_window`, so that
        event_list / event_list_pol_mask / event_mask are the slices [:, p] of window buffers; `reset`: the loop reset
        model, loss and gradients in front of the first of them.  Batches the loop forwards and drops are not returned;
        their hot-pixel observations are made."""
        discarded, group, reset = self.plan_window(P)
        self.observe(discarded)
        passes = self.window_passes(group)
        self.new_seq, self.pass_done = reset, group[-1][2]
        return passes, reset

    def observe(self, discarded):
        """Batches the loop forwarded and dropped: their hot-pixel statistics only; masks and rows are dropped."""
        if self.hot:
            for at in range(0, len(discarded), 64):
                self._cut(discarded[at:at + 64])


class StaticTable:
    """A job table at a fixed device address that is rewritten step after step (a captured graph reads fixed addresses): the
    `base` int64 words of the loader's `_job_table`, then `extra_words` of the caller's, and a ring of pinned host tables, each
    with an event recorded after its copy: the host waits on it before rewriting the table."""

    RING = 4  # pinned job tables in flight (>= 2)

    def __init__(self, loader, base, extra_words=0):
        self.loader, self.base = loader, int(base)
        words = self.base + int(extra_words)
        self.table_dev = torch.empty(words, dtype=torch.int64, device=loader.device)
        self.ring = [(torch.empty(words, dtype=torch.int64).pin_memory(), torch.cuda.Event()) for _ in range(self.RING)]

    def stage(self, group, seen):
        """Step `seen`'s pinned table with `_job_table(group)` in its prefix -> the host view of the extra words, for the
        caller to fill before `send`."""
        self._staged = pinned, copied = self.ring[seen % self.RING]
        copied.synchronize()
        host = pinned.numpy()
        host[:self.base] = self.loader._job_table(group)
        return host[self.base:]

    def send(self):
        """The staged table to the device on the current stream (non-blocking)."""
        pinned, copied = self._staged
        self.table_dev.copy_(pinned, non_blocking=True)
        copied.record()


class ResidentWindow(StaticTable):
    """The static buffers of a window of P batches that is cut again and again: the loader's `_buffers(P)`, dt_gt zeros [P,B]
    and `StaticTable` over `_job_table`'s 2*B*P + 1 int64 words."""

    def __init__(self, loader, P, extra_words=0):
        self.P = int(P)
        self.static_ev, self.dt, self.m_bp, self.m_pb = loader._buffers(self.P)
        self.dt_gt = torch.zeros((self.P, loader.batch_size), dtype=torch.float64, device=loader.device)
        super().__init__(loader, 2 * loader.batch_size * self.P + 1, extra_words)

    def launch(self):
        """The cut, the hot-pixel kernel, the binning and the mask launches on the static buffers -> the window's passes.  No
        allocation beyond `encode_window`'s: it runs under capture."""
        self.loader._launch_cut(self.table_dev, self.P, self.static_ev, self.dt, self.m_bp, self.m_pb)
        return self.loader._window_passes(self.static_ev, self.dt, self.m_bp, self.m_pb, self.dt_gt)


def zero_states_if(flag_ptr, states):
    """The tensors of `states` (a model's `state_buffers()`) zero-filled when the int32 at device address `flag_ptr` is not 0:
    evf_zero_segments_if, 32 segments a launch -- `model.reset_states()` as a node of a captured graph."""
    flat = [t for st in states if st is not None for t in st if t is not None]
    for lo in range(0, len(flat), 32):
        seg = flat[lo:lo + 32]
        _lib.call("evf_zero_segments_if", flag_ptr, (ctypes.c_void_p * 32)(*[_lib.ptr(t) for t in seg]),
                  (ctypes.c_int64 * 32)(*[t.numel() * t.element_size() for t in seg]), len(seg))

