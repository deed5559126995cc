"""Device-resident event sequences: every sequence file of the loader's shard is uploaded ONCE, and every batch -- or every
whole BPTT window -- is then cut, formatted, flipped, filtered and binned by kernels (csrc/evf_resident.hip + the existing
binning), with the keys, shapes, dtypes and values `H5Loader` gives on the same files, flags and RNG state.

Only `data.mode: events` (the training mode): there the next window of a slot is index arithmetic on the sequence LENGTHS,
so the host decides everything without a device value.  That decision is `ResidentPlan` -- H5Loader's own constructor, file
list, sharding, augmentation flags, `reset_sequence`, `shuffle`, counters and `_end_pass`, plus the cursor step of
dataloader/h5.py:244-279,310 written over lengths.  It needs no GPU.  `ResidentLoader` adds the arena and the launches.

Layout in device memory: one arena per column over all files, `xs`, `ys` uint16, `ts` float64 RELATIVE to its file's t0
(subtracted on the host in float64 exactly like `get_events`), `ps` uint8 -- 13 bytes per event -- and int64 offsets."""

import numpy as np
import torch

from .. import _lib
from .encodings import encode_event_list, encode_window
from .h5 import H5Loader, open_sequence

FLAG_BITS = (("Horizontal", 1), ("Vertical", 2), ("Polarity", 4))


class ResidentPlan(H5Loader):
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

    def _open(self, batch, path):  # (H5Loader opens the slot's file here; a plan only notes which one it is)
        self._slot_path[batch] = path

    def _read_lengths(self):
        out = {}
        for path in self.files:
            seq = open_sequence(path)
            out[path] = len(seq.events("xs"))
            seq.close()
        return out

    def slot_flags(self, batch):
        return sum(bit for mech, bit in FLAG_BITS if self._flipped(mech, batch))

    def plan_sample(self, batch):
        """dataloader/h5.py:244-279,310 for one slot -> (path, first event, flags, restarted)."""
        restarted = False
        while self.lengths[self._slot_path[batch]] - self.batch_row[batch] < self.window:  # fewer events left than a window
            restarted = self._restarted = True
            if not self._threaded:
                self.new_seq = True
            self.reset_sequence(batch)
            self.batch_row[batch] = 0
            self.batch_idx[batch] = max(self.batch_idx) + 1
            self._open(batch, self.files[self.batch_idx[batch] % len(self.files)])
        first = self.batch_row[batch]
        self.batch_row[batch] += self.window
        return self._slot_path[batch], first, self.slot_flags(batch), restarted

    def plan_batches(self):
        """`H5Loader._host_batches` over the plan: ([job of slot 0, ...], (a slot restarted, wrap-around batch)) until
        every file has been started once."""
        while True:
            self._restarted = False
            jobs = [self.plan_sample(b) for b in range(self.batch_size)]
            done = self.seq_num >= len(self.files)
            yield jobs, (self._restarted, done)
            if done:
                return

    def _endless(self):
        """The batches of pass after pass over the files, as the training driver meets them: (jobs, restarted, done)."""
        while True:
            for jobs, (restarted, done) in self.plan_batches():
                self.new_seq, self.pass_done = restarted, done  # (H5Loader._deliver's bookkeeping)
                self.samples += self.batch_size
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
                self.new_seq, self.pass_done = restarted, done
                self.samples += self.batch_size
                if done:
                    break
                group.append((jobs, restarted, done))
                if len(group) == P:
                    yield group, [r for _j, r, _d in group], False
                    group = []
            yield group, [r for _j, r, _d in group], True
        finally:
            self._end_pass()


class ResidentLoader(ResidentPlan):
    def __init__(self, config, num_bins, round_encoding=False, device=None, rank=0, world_size=1):
        super().__init__(config, num_bins, round_encoding, device, rank, world_size)  # (reads the columns: _read_lengths)
        cols, self._cols = self._cols, None
        _lib.load()  # the refusals above are host work; from here on the device
        if not torch.cuda.is_available():
            raise _lib.EvflowError("ResidentLoader: the sequences live and are cut on the MI355X only (no CPU fallback)")
        dev = self.device
        self.offsets, at = {}, 0
        for path in self.files:
            self.offsets[path] = at
            at += self.lengths[path]
        self.total_events = at
        self._xs, self._ys, self._ts, self._ps = (torch.from_numpy(np.concatenate(c)).to(dev) for c in cols)
        self.resident_bytes = sum(t.numel() * t.element_size() for t in (self._xs, self._ys, self._ts, self._ps))
        H, W = self.res
        self.hot = bool(self.config["hot_filter"]["enabled"])
        if self.hot:
            self._hot_events = torch.zeros((self.batch_size, H, W), dtype=torch.int32, device=dev)
            self._hot_obvs = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
        self._last_row = None
        self._last_ts = 0

    def _read_lengths(self):
        """Every file's four columns, once (kept in self._cols until they are uploaded) -> their lengths."""
        xs, ys, ts, ps, lengths = [], [], [], [], {}
        for path in self.files:
            seq = open_sequence(path)
            x, y, p = (np.asarray(seq.events(k)[:]) for k in ("xs", "ys", "ps"))
            t = np.asarray(seq.events("ts")[:], dtype=np.float64) - seq.attrs["t0"]  # get_events, h5.py:210
            seq.close()
            for name, c in (("xs", x), ("ys", y)):
                if c.size and not (np.all(c == np.floor(c)) and c.min() >= 0 and c.max() <= 65535):
                    raise _lib.EvflowError(f"{path}: events/{name} holds values that are no integers in [0, 65535]; the "
                                           "resident arena stores uint16 coordinates: use H5Loader")
            if p.size and not np.all((p == 0) | (p == 1)):
                raise _lib.EvflowError(f"{path}: events/ps holds polarities outside {{0, 1}}: use H5Loader")
            lengths[path] = len(x)
            xs.append(x.astype(np.uint16))
            ys.append(y.astype(np.uint16))
            ts.append(t)
            ps.append(p.astype(np.uint8))
        self._cols = (xs, ys, ts, ps)
        return lengths

    # ------------------------------------------------------------------ launches
    def _job_table(self, batches):
        """The host table of P planned batches, job j = b * P + p: `first` int64 [B*P], then as int32 `flags` [B*P] | slot
        `reset` [B*P] | the window's `reset` (did the first batch restart a slot: train_flow.py's loop reset the model in front
        of it) -- one int64 array of 2*B*P + 1 words."""
        B, P, N = self.batch_size, len(batches), self.window
        tab = np.zeros(2 * B * P + 1, dtype=np.int64)
        aux = tab[B * P:].view(np.int32)
        for p, (jobs, _restarted, _done) in enumerate(batches):
            for b, (path, first, flags, restarted) in enumerate(jobs):
                tab[b * P + p] = self.offsets[path] + first
                aux[b * P + p] = flags
                aux[B * P + b * P + p] = 1 if restarted else 0
        aux[2 * B * P] = 1 if batches[0][1] else 0
        self._last_row = int(tab[B * P - 1]) + N - 1  # last event of the last slot's last pass
        return tab

    def _launch_cut(self, table_dev, P, ev, dt, m_bp=None, m_pb=None):
        """evf_seq_cut and, with the hot filter, evf_hot_pixels on a job table in device memory (`_job_table`'s layout), into
        the caller's ev [B,P,N,4], dt [P,B] float64 and masks m_bp [B,P,H,W] / m_pb [P,B,H,W] (either may be None).  No
        allocation and no host copy: the launches can be captured."""
        B, N = self.batch_size, self.window
        H, W = self.res
        at = table_dev.data_ptr()
        _lib.call("evf_seq_cut", _lib.ptr(self._xs), _lib.ptr(self._ys), _lib.ptr(self._ts), _lib.ptr(self._ps), self.total_events,
                  at, at + 8 * B * P, B, P, N, H, W, _lib.ptr(ev), _lib.ptr(dt))
        if self.hot:
            hf = self.config["hot_filter"]
            _lib.call("evf_hot_pixels", _lib.ptr(ev), at + 12 * B * P, _lib.ptr(self._hot_events), _lib.ptr(self._hot_obvs),
                      _lib.ptr(m_bp), _lib.ptr(m_pb), B, P, N, H, W, int(hf["max_px"]), int(hf["min_obvs"]), float(hf["max_rate"]))

    def _cut(self, batches):
        """P planned batches -> ev [B,P,N,4], dt_input [P,B], hot masks ([B,P,H,W], [P,B,H,W]) or None: one copy of the job
        table, one evf_seq_cut, one evf_hot_pixels."""
        B, P, N = self.batch_size, len(batches), self.window
        H, W = self.res
        dev = self.device
        t = torch.from_numpy(self._job_table(batches))
        t = t.pin_memory().to(dev, non_blocking=True)
        ev = torch.empty((B, P, N, 4), dtype=torch.float32, device=dev)
        dt = torch.empty((P, B), dtype=torch.float64, device=dev)
        m_bp = m_pb = None
        if self.hot:
            m_bp = torch.empty((B, P, H, W), dtype=torch.float32, device=dev)
            m_pb = torch.empty((P, B, H, W), dtype=torch.float32, device=dev) if P > 1 else None  # (P = 1: the same layout)
        self._launch_cut(t, P, ev, dt, m_bp, m_pb)
        masks = (m_bp, m_pb if m_pb is not None else m_bp.view(P, B, H, W)) if self.hot else None
        return ev, dt, masks

    def _mask_window(self, passes, m_bp, m_pb):
        """The hot-pixel masks applied in place to the window buffers behind `passes` (encode_window's dicts)."""
        B, P = self.batch_size, len(passes)
        H, W = self.res
        # network inputs are pass-major ([P,B,C,H,W], one tensor per pass), the loss's mask stack batch-major ([B,P,H,W])
        cnt = torch.as_strided(passes[0]["event_cnt"], (P * B, 2, H, W), passes[0]["event_cnt"].stride())
        vox = torch.as_strided(passes[0]["event_voxel"], (P * B, self.num_bins, H, W), passes[0]["event_voxel"].stride())
        emask = torch.as_strided(passes[0]["event_mask"], (B * P, 1, H, W), (H * W, H * W, W, 1))
        _lib.call("evf_apply_pixel_mask", _lib.ptr(vox), _lib.ptr(m_pb), P * B, self.num_bins, H, W)
        _lib.call("evf_apply_pixel_mask", _lib.ptr(cnt), _lib.ptr(m_pb), P * B, 2, H, W)
        _lib.call("evf_apply_pixel_mask", _lib.ptr(emask), _lib.ptr(m_bp), B * P, 1, H, W)

    def _produce(self, batch):
        """One planned batch -> the reference's batch dict (dataloader/base.py:248-265)."""
        B = self.batch_size
        H, W = self.res
        ev, dt, masks = self._cut([batch])
        out = encode_event_list(ev.view(B, self.window, 4), self.num_bins, self.res, round_ts=self.round_encoding)
        if masks is not None:
            for key, C in (("event_voxel", self.num_bins), ("event_cnt", 2), ("event_mask", 1)):
                _lib.call("evf_apply_pixel_mask", _lib.ptr(out[key]), _lib.ptr(masks[0]), B, C, H, W)
        out["dt_gt"] = torch.zeros(B, dtype=torch.float64, device=self.device)
        out["dt_input"] = dt[0]
        return out

    def __iter__(self):
        """The batches of one pass over the files, like `H5Loader.__iter__` with its flags: no reader thread, no device
        synchronisation."""
        try:
            for jobs, (restarted, done) in self.plan_batches():
                batch = self._produce((jobs, restarted, done))
                self.new_seq, self.pass_done = restarted, done
                self.samples += self.batch_size
                yield batch
        finally:
            self._end_pass()

    def next_window(self, P):
        """-> (passes, reset): the P batch dicts of the next group of batches on which train_flow.py's loop steps the
        optimizer (see `plan_window`), cut by ONE launch into one [B,P,N,4] buffer and binned by `encode_window`, so that
        event_list / event_list_pol_mask / event_mask are the slices [:, p] of window buffers; `reset`: the loop reset
        model, loss and gradients in front of the first of them.  Batches the loop forwards and drops are not returned;
        their hot-pixel observations are made."""
        discarded, group, reset = self.plan_window(P)
        if self.hot:
            for at in range(0, len(discarded), 64):  # statistics only; masks and rows are dropped
                self._cut(discarded[at:at + 64])
        B = self.batch_size
        ev, dt, masks = self._cut(group)
        passes = encode_window(ev, self.num_bins, self.res, round_ts=self.round_encoding)
        if masks is not None:
            self._mask_window(passes, *masks)
        zeros = torch.zeros((P, B), dtype=torch.float64, device=self.device)
        for p, d in enumerate(passes):
            d["dt_gt"] = zeros[p]
            d["dt_input"] = dt[p]
        self.new_seq, self.pass_done = reset, group[-1][2]
        return passes, reset

    # ------------------------------------------------------------------ one value on demand
    @property
    def last_proc_timestamp(self):
        """Timestamp (relative to its file's t0) of the last event handed out: fetched from the arena when asked for."""
        if self._last_row is not None:
            self._last_ts = float(self._ts[self._last_row])
            self._last_row = None
        return self._last_ts

    @last_proc_timestamp.setter
    def last_proc_timestamp(self, value):
        self._last_row, self._last_ts = None, value
