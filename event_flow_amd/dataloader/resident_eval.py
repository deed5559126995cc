"""Device-resident evaluation: `data.mode` `time`, `frames`, `gtflow_dt1` and `gtflow_dt4` on sequence files that are uploaded
ONCE -- the modes the reference evaluates with (AEE needs the ground-truth modes).  Every batch is cut, formatted, flipped,
filtered and binned by kernels (csrc/evf_resident_eval.hip, csrc/evf_resident.hip + the existing binning) and carries the keys,
shapes, dtypes and values `H5Loader` gives on the same files, config and RNG state; `gtflow` / `frames` are gathered and flipped
from maps and frames that live in device memory.  `data.mode: events` stays with dataloader/resident.py.

Two things make these modes differ from `events`: a window's borders are TIMESTAMPS, found by `binary_search_array`, and the
windows of a batch hold different numbers of events.  Both are settled on the host without a device value:

  * Every border a file can ever be asked for is known when the file is opened -- the stamps of the configured group, or in
    `time` mode the cursor values 0, w, w + w, ... (+ t0) up to the file's last event.  `boundary_queries` lists them, ONE
    `evf_ts_search` launch at construction answers all of them for all files, and the table comes back to the host (the only
    device-to-host copy).  The search runs on the files' ABSOLUTE float64 timestamps, like `H5Loader.find_ts_index`; that
    column is needed for this one search only and is freed after it, so it is not part of `resident_bytes`.
  * With the table on the host, the host knows every window's first event and event count before the launch: the padded
    width of a batch is `max(count)`, and "up to 10 events is an empty window" (dataloader/h5.py:268) is `count = 0`.

`ResidentEvalPlan` is the host-only half (no GPU): `ResidentCursor` (dataloader/resident_base.py, shared with the `events`
loader) plus `__getitem__`'s cursor step (dataloader/h5.py:243-311) written over the tables.  `ResidentEvalLoader` adds the
arenas and the launches.

Layout in device memory: the 13-byte event arena of `ResidentArena` (dataloader/resident_base.py), and for the mode's group
either the ground-truth maps
`[M,2,H,W]` float32 (8 H W bytes per map) or the frames `[M,H,W]` uint8 (H W bytes per frame), all files' in file order, a
file's in the order of `_Sequence.group()`."""

import numpy as np
import torch

from .. import _lib
from .encodings import binary_search_array, encode_event_list
from .h5 import open_sequence
from .resident import StaticTable
from .resident_base import ResidentArena, ResidentCursor, read_columns

MODES = ("time", "frames", "gtflow_dt1", "gtflow_dt4")


class ResidentEvalPlan(ResidentCursor):
    """The host-only half: per slot (sequence file, first event, event count, flip flags, restarted, map index or frame indices,
    dt_gt) of the next input window -- the decisions, counters and `np.random.random()` draws of `H5Loader.__getitem__`, in
    its order.

    meta: path -> {"events": count, "t0", "duration", "last_ts": last timestamp - t0, "names", "stamps": the mode's group};
    read from the files when omitted.  index: path -> int64 array, `binary_search_array(events/ts, q)` for every q of
    `boundary_queries(path)`; searched on the host when omitted (the loader searches on the device instead)."""

    def __init__(self, config, num_bins, round_encoding=False, device=None, rank=0, world_size=1, meta=None, index=None):
        mode, window = config["data"]["mode"], config["data"]["window"]
        if mode == "events":
            raise _lib.EvflowError("ResidentEvalLoader serves data.mode 'time', 'frames', 'gtflow_dt1' and 'gtflow_dt4'; windows by "
                                   "event count are ResidentLoader's (or H5Loader's)")
        if mode in MODES and (isinstance(window, bool) or not window > 0):
            raise _lib.EvflowError(f"ResidentEvalLoader needs a data.window > 0, got {window!r}: use H5Loader")
        self._slot_path, self._slot_step = {}, {}
        super().__init__(config, num_bins, round_encoding, device, prefetch=0, rank=rank, world_size=world_size)
        self.last_row = None  # (path, event index) behind `last_proc_timestamp`: last event of the last non-empty slice
        self.meta = dict(meta) if meta is not None else self._read_meta()
        for path in self.files:
            if self._stamp_group() and not len(self.meta[path]["stamps"]):
                raise _lib.EvflowError(f"{path}: no group '{self._stamp_group()}' for data.mode '{self.mode}': use H5Loader "
                                       "on files that carry it")
        self.queries = {path: self.boundary_queries(path) for path in self.files}
        self.index = dict(index) if index is not None else self._search()
        for path in self.files:
            if len(self.index[path]) != len(self.queries[path]):
                raise _lib.EvflowError(f"{path}: index table of {len(self.index[path])} entries for {len(self.queries[path])} "
                                       "boundary queries")

    def _open(self, batch, path):  # (the plan notes the slot's file and rewinds)
        super()._open(batch, path)
        self._slot_step[batch] = 0  # windows handed out (or tried) since the file was opened: the row of the time table

    # ------------------------------------------------------------------ what the files say
    def _group_of(self, seq, path):
        g = self._stamp_group()
        if g is None:
            return [], []
        try:
            names, stamps = seq.group(g)
        except Exception:  # (h5py: KeyError, the ctypes reader: its own error -- a file without the group either way)
            names, stamps = [], []
        if not len(names):
            raise _lib.EvflowError(f"{path}: no group '{g}' for data.mode '{self.mode}': use H5Loader on files that carry it")
        return list(names), list(stamps)

    def _read_meta(self):
        out = {}
        for path in self.files:
            seq = open_sequence(path)
            names, stamps = self._group_of(seq, path)
            out[path] = {"events": len(seq.events("xs")), "t0": seq.attrs["t0"], "duration": seq.attrs["duration"],
                         "last_ts": seq.events("ts")[-1] - seq.attrs["t0"], "names": names, "stamps": stamps}
            seq.close()
        return out

    def boundary_queries(self, path):
        """Every timestamp `find_ts_index` can be asked for on this file, float64: the stamps of the group, or in `time` mode
        the pair (row + t0, row + t0 + window) of every window, row = 0 and then `+= window` like the cursor, up to and with the
        window that makes the slot move on (h5.py:232-234,264)."""
        m = self.meta[path]
        if self.mode != "time":
            return np.asarray([float(s) for s in m["stamps"]], dtype=np.float64)
        q, row = [], 0
        while True:
            t = row + m["t0"]
            q += [t, t + self.window]
            if row + self.window >= m["last_ts"]:
                break
            if row + self.window == row or len(q) > (1 << 26):
                raise _lib.EvflowError(f"{path}: a data.window of {self.window!r} s does not advance through a sequence of "
                                       f"{m['last_ts']!r} s: use H5Loader")
            row += self.window
        return np.asarray(q, dtype=np.float64)

    def _search(self):
        """The index tables by the reference's own search on the host (the loader overrides this with one evf_ts_search)."""
        out = {}
        for path in self.files:
            seq = open_sequence(path)
            ts = np.asarray(seq.events("ts")[:], dtype=np.float64)
            seq.close()
            out[path] = np.asarray([binary_search_array(ts, q) for q in self.queries[path]], dtype=np.int64)
        return out

    # ------------------------------------------------------------------ the cursor
    def _event_range(self, batch):
        """`get_event_index` + the sub-interval arithmetic of h5.py:254-260 over the index table -> (idx0, idx1)."""
        path = self._slot_path[batch]
        table = self.index[path]
        if self.mode == "time":
            k = self._slot_step[batch]
            return int(table[2 * k]), int(table[2 * k + 1])
        row0, row1 = self._stamp_rows(batch, self.window)
        idx0, idx1 = int(table[row0]), int(table[row1])
        if self.window < 1.0:
            idx0_change = self.batch_row[batch] - row0
            idx1_change = self.batch_row[batch] + self.window - row0
            delta_idx = idx1 - idx0
            idx1 = int(idx0 + idx1_change * delta_idx)
            idx0 = int(idx0 + idx0_change * delta_idx)
        return idx0, idx1

    def plan_sample(self, batch):
        """dataloader/h5.py:243-311 for one slot -> (path, first event, event count, flags, restarted, indices, dt_gt);
        indices: the map's index in its file's group (gtflow modes), (curr, next) frame indices (frames), None (time)."""
        stamped = self.mode != "time"
        restarted = False
        while True:
            path = self._slot_path[batch]
            m = self.meta[path]
            row = self.batch_row[batch]
            restart = stamped and int(np.ceil(row + self.window)) >= len(m["stamps"])
            first = count = 0
            if not restart:
                idx0, idx1 = self._event_range(batch)
                n = m["events"]  # the slice [idx0:idx1] of n events
                first = min(max(idx0, 0), n)
                count = max(min(max(idx1, 0), n) - first, 0)
                if count > 0:  # get_events, h5.py:212-213 -- before the restart test and the rule below
                    self.last_row = (path, first + count - 1)
            if self.mode == "time" and row + self.window >= m["last_ts"]:
                restart = True
            if count <= 10:  # very few events: an empty window (h5.py:268)
                count = 0
            if restart:
                restarted = True
                self._restart(batch)
                continue
            indices, dt_gt = None, 0.0
            if self.mode == "frames":
                indices = (int(np.floor(row)), int(np.ceil(row + self.window)))
            elif stamped:
                indices = int(np.ceil(row + self.window))
                if indices > 0:
                    dt_gt = m["stamps"][indices] - m["stamps"][indices - 1]
            self.batch_row[batch] += self.window
            self._slot_step[batch] += 1
            return path, first, count, self.slot_flags(batch), restarted, indices, float(dt_gt)

    def plan_eval_passes(self):
        """ONE pass over the files as eval_flow.py's loop meets it in a ground-truth mode with AEE: the batches of
        `plan_batches()` up to, not including, the wrap-around (`done`) batch -- the loop breaks on that one before forwarding
        it -- as (jobs, restarted, evaluate) per batch.  `restarted`: the loop's `model.reset_states()` in front of the pass;
        `evaluate`: the loop's `idx_AEE` rule over host values -- a batch whose slot-0 dt_gt <= 0 neither counts nor evaluates,
        every other one counts, and the batch on which the counter reaches round(1 / window) evaluates and returns it to 0
        (reference eval_flow.py:169-176).  The loader's flags, sample counter and end-of-pass bookkeeping move as in
        `__iter__`, np.random is drawn from exactly as there."""
        if self.mode not in ("gtflow_dt1", "gtflow_dt4"):
            raise _lib.EvflowError(f"plan_eval_passes: AEE is evaluated on ground-truth windows (gtflow_dt1 / gtflow_dt4), not in "
                                   f"data.mode '{self.mode}'")
        aee_every = int(np.round(1.0 / self.window))
        counted = 0
        try:
            for jobs, (restarted, done) in self.plan_batches():
                self._delivered(restarted, done)
                if done:
                    break
                evaluate = False
                if not jobs[0][6] <= 0.0:
                    counted += 1
                    if counted == aee_every:
                        evaluate, counted = True, 0
                yield jobs, restarted, evaluate
        finally:
            self._end_pass()


class ResidentEvalLoader(ResidentArena, ResidentEvalPlan):
    """`resident_bytes`: everything kept in device memory -- 13 bytes per event, 8 H W per ground-truth map or H W per frame
    (a sequence of a few thousand 260 x 346 maps is gigabytes), the hot-pixel statistics.  The absolute timestamp column of the
    one search at construction (8 bytes per event) is freed after it and not counted."""

    def __init__(self, config, num_bins, round_encoding=False, device=None, rank=0, world_size=1):
        super().__init__(config, num_bins, round_encoding, device, rank, world_size)  # (_read_meta, then _search on the device)
        cols, self._cols = self._cols, None
        dev = self.device
        H, W = self.res
        self._upload(cols)
        self._stack = None  # the mode's maps [M,2,H,W] float32 or frames [M,H,W] uint8
        if self._stamp_group():
            self.stack_offsets, at = {}, 0
            for path in self.files:
                self.stack_offsets[path] = at
                at += len(self.meta[path]["names"])
            self.stack_items = at
            shape, dtype = ((at, H, W), torch.uint8) if self.mode == "frames" else ((at, 2, H, W), torch.float32)
            self._stack = torch.empty(shape, dtype=dtype, device=dev)
            for path in self.files:  # (one upload per file, no second copy of everything on either side)
                a = self._items.pop(path)
                self._stack[self.stack_offsets[path]:self.stack_offsets[path] + len(a)].copy_(torch.from_numpy(a))
            self.resident_bytes += self._stack.numel() * self._stack.element_size()
        if self.hot:
            self.resident_bytes += 4 * (self._hot_events.numel() + self._hot_obvs.numel())

    # ------------------------------------------------------------------ construction
    def _read_meta(self):
        """Every file of the shard once: the four columns (kept in self._cols until they are uploaded; the absolute timestamps
        in self._ts_abs until the search), the group's maps or frames (self._items), the metadata of the plan."""
        H, W = self.res
        g = self._stamp_group()
        self._cols, self._ts_abs, self._items, meta = ([], [], [], []), [], {}, {}
        for path in self.files:
            seq = open_sequence(path)
            names, stamps = self._group_of(seq, path)
            *cols, ta = read_columns(seq, path)
            if not len(ta):
                raise _lib.EvflowError(f"{path}: no events: use H5Loader")
            items = []
            for name in names:
                a = seq.read(g, name)
                want = (H, W) if self.mode == "frames" else (2, H, W)
                if tuple(np.shape(a)) != want:
                    raise _lib.EvflowError(f"{path}: {g}/{name} has shape {tuple(np.shape(a))}, the loader resolution needs "
                                           f"{want}: use H5Loader")
                # frames: a float64 buffer cast to uint8 (h5.py:295-298); maps: augment_flowmap's float32 copy
                items.append(np.asarray(a, dtype=np.float64).astype(np.uint8) if self.mode == "frames" else
                             np.array(a, dtype=np.float32))
            if items:
                self._items[path] = np.stack(items)
            meta[path] = {"events": len(ta), "t0": seq.attrs["t0"], "duration": seq.attrs["duration"],
                          "last_ts": seq.events("ts")[-1] - seq.attrs["t0"], "names": names, "stamps": stamps}
            seq.close()
            for col, c in zip(self._cols, cols):
                col.append(c)
            self._ts_abs.append(ta)
        self._place({path: m["events"] for path, m in meta.items()})
        return meta

    def _search(self):
        """Every boundary query of every file in one evf_ts_search on the absolute timestamps -> the plan's index tables.
        Everything before this was host work (the refusals); this is the first device work and the only copy back."""
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.EvflowError("ResidentEvalLoader: the sequences live and are cut on the MI355X only (no CPU fallback)")
        dev = self.device
        ts_abs, self._ts_abs = self._ts_abs, None
        begin = np.concatenate([np.full(len(self.queries[p]), self.offsets[p], dtype=np.int64) for p in self.files])
        length = np.concatenate([np.full(len(self.queries[p]), self.meta[p]["events"], dtype=np.int64) for p in self.files])
        query = np.concatenate([self.queries[p] for p in self.files])
        col = torch.from_numpy(np.concatenate(ts_abs)).to(dev)
        b, n, q = (torch.from_numpy(a).to(dev) for a in (begin, length, query))
        out = torch.empty(len(query), dtype=torch.int64, device=dev)
        _lib.call("evf_ts_search", _lib.ptr(col), self.total_events, _lib.ptr(b), _lib.ptr(n), _lib.ptr(q), len(query), _lib.ptr(out))
        found = out.cpu().numpy()
        del col
        if (found < 0).any():
            raise _lib.EvflowError("evf_ts_search: a segment outside the timestamp column")
        tables, at = {}, 0
        for p in self.files:
            tables[p] = found[at:at + len(self.queries[p])]
            at += len(self.queries[p])
        return tables

    # ------------------------------------------------------------------ launches
    def _job_table(self, jobs):
        """The host table of one planned batch as int64 words: `first` int64 [B] | `dt_gt` float64 [B] | as int32 `count` [B],
        `flags` [B], `reset` [B], two index columns [B] each (map index, or curr and next frame; into the resident stack)."""
        B = self.batch_size
        tab = np.zeros(2 * B + (5 * B + 1) // 2, dtype=np.int64)
        dt_gt = tab[B:2 * B].view(np.float64)
        aux = tab[2 * B:].view(np.int32)
        for b, (path, first, count, flags, restarted, indices, dt) in enumerate(jobs):
            tab[b] = self.offsets[path] + first
            dt_gt[b] = dt
            aux[b], aux[B + b], aux[2 * B + b] = count, flags, 1 if restarted else 0
            if indices is not None:
                i0, i1 = indices if isinstance(indices, tuple) else (indices, indices)
                aux[3 * B + b], aux[4 * B + b] = self.stack_offsets[path] + i0, self.stack_offsets[path] + i1
        return tab

    def _produce(self, jobs, _restarted=False, _done=False):
        """One planned batch -> the reference's batch dict (dataloader/base.py:248-265): one copy of the job table, then the
        cut, the hot-pixel filter, the binning, the masks and the gather."""
        npad = max(j[2] for j in jobs)  # known on the host: no device value decides a shape
        N = max(npad, 1)
        t = torch.from_numpy(self._job_table(jobs)).pin_memory().to(self.device, non_blocking=True)
        out = self._launch(t, N, *self._buffers(N))
        if npad == 0:  # only padding rows: empty lists, like custom_collate
            out["event_list"] = out["event_list"][:, :0]
            out["event_list_pol_mask"] = out["event_list_pol_mask"][:, :0]
        return out

    def _buffers(self, N):
        """The buffers of a batch of width N: ev [B,N,4], dt_input [B] float64, with the hot filter the mask [B,H,W], and the
        mode's gathered maps [B,2,H,W] float32 or frames [B,2,H,W] uint8 (None in `time` mode)."""
        B, dev = self.batch_size, self.device
        H, W = self.res
        ev = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
        dt = torch.empty(B, dtype=torch.float64, device=dev)
        mask = torch.empty((B, H, W), dtype=torch.float32, device=dev) if self.hot else None
        items = None
        if self._stack is not None:
            items = torch.empty((B, 2, H, W), dtype=torch.uint8 if self.mode == "frames" else torch.float32, device=dev)
        return ev, dt, mask, items

    def _launch(self, table_dev, N, ev, dt, mask, items):
        """The launches of one batch on a job table in device memory (`_job_table`'s layout) into the caller's `_buffers(N)`:
        the ragged cut (rows behind a slot's count are zero, whatever N), the hot-pixel kernel with its reset column, the
        binning, the masks and the gather -> the batch dict, `dt_gt` a view of the table.  No allocation beyond
        `encode_event_list`'s and no host copy: the launches can be captured."""
        B = self.batch_size
        H, W = self.res
        at = table_dev.data_ptr()
        aux = at + 16 * B
        _lib.call("evf_seq_cut_ragged", _lib.ptr(self._xs), _lib.ptr(self._ys), _lib.ptr(self._ts), _lib.ptr(self._ps),
                  self.total_events, at, aux, aux + 4 * B, B, N, H, W, _lib.ptr(ev), _lib.ptr(dt))
        if self.hot:  # (an empty window is an observation too, like create_hot_mask's)
            _lib.call("evf_hot_pixels", _lib.ptr(ev), aux + 8 * B, _lib.ptr(self._hot_events), _lib.ptr(self._hot_obvs), _lib.ptr(mask),
                      None, B, 1, N, H, W, *self._hot_params())
        out = encode_event_list(ev, self.num_bins, self.res, round_ts=self.round_encoding)
        if self.hot:
            self._mask_batch(out, mask)
        out["dt_gt"] = table_dev[B:2 * B].view(torch.float64)
        out["dt_input"] = dt
        if self.mode == "frames":
            out["frames"] = items
            _lib.call("evf_gather_frames", _lib.ptr(self._stack), self.stack_items, aux + 12 * B, aux + 16 * B, aux + 4 * B, B, H, W,
                      _lib.ptr(items))
        elif self._stack is not None:
            out["gtflow"] = items
            _lib.call("evf_gather_flowmaps", _lib.ptr(self._stack), self.stack_items, aux + 12 * B, aux + 4 * B, B, H, W,
                      _lib.ptr(items))
        return out


class ResidentEvalWindow(StaticTable):
    """The static buffers of ONE batch of a fixed width that is produced again and again (a captured graph reads fixed
    addresses): the loader's `_buffers(capacity)`, the job table in device memory -- `_job_table`'s 2 B + ceil(5 B / 2) int64
    words, then `extra_words` of the caller's -- and `StaticTable`'s ring of pinned host tables.  `capacity`: at least the
    largest event count of any job that will be staged; the rows behind a slot's count are zero, so the padding is invisible
    to the binning, the masks and the hot-pixel statistics."""

    def __init__(self, loader, capacity, extra_words=0):
        self.capacity = max(int(capacity), 1)
        self.buffers = loader._buffers(self.capacity)
        B = loader.batch_size
        super().__init__(loader, 2 * B + (5 * B + 1) // 2, extra_words)

    def stage(self, jobs, seen):
        most = max(j[2] for j in jobs)
        if most > self.capacity:
            raise _lib.EvflowError(f"ResidentEvalWindow: a window of {most} events in buffers of {self.capacity}")
        return super().stage(jobs, seen)

    def launch(self):
        """`ResidentEvalLoader._launch` on the static buffers -> the batch dict (event lists of `capacity` rows)."""
        return self.loader._launch(self.table_dev, self.capacity, *self.buffers)
