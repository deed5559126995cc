"""What the device-resident loaders share (dataloader/resident.py: `events`; dataloader/resident_eval.py: the evaluation modes):
`ResidentCursor`, the host-only cursor over H5Loader's counters, `read_columns`, what a resident file may contain, and
`ResidentArena`, the 13-byte event arena in device memory with the hot-pixel statistics."""

import numpy as np
import torch

from .. import _lib
from .h5 import H5Loader

FLAG_BITS = (("Horizontal", 1), ("Vertical", 2), ("Polarity", 4))


def read_columns(seq, path):
    """The four event columns of an open sequence as the arena stores them -> (xs uint16, ys uint16, ts float64 RELATIVE to the
    file's t0 -- subtracted in float64 like `get_events`, h5.py:210 --, ps uint8, the absolute ts float64)."""
    x, y, p = (np.asarray(seq.events(k)[:]) for k in ("xs", "ys", "ps"))
    ta = np.asarray(seq.events("ts")[:], dtype=np.float64)
    for name, c in (("xs", x), ("ys", y)):
        if c.size and not (np.all(c == np.floor(c)) and c.min() >= 0 and c.max() <= 65535):
            raise _lib.EvflowError(f"{path}: events/{name} holds values that are no integers in [0, 65535]; the "
                                   "resident arena stores uint16 coordinates: use H5Loader")
    if p.size and not np.all((p == 0) | (p == 1)):
        raise _lib.EvflowError(f"{path}: events/ps holds polarities outside {{0, 1}}: use H5Loader")
    return x.astype(np.uint16), y.astype(np.uint16), ta - seq.attrs["t0"], p.astype(np.uint8), ta


class ResidentCursor(H5Loader):
    """The host-only half of both plans: H5Loader's constructor, file list, sharding, flags, `reset_sequence`, `shuffle`,
    counters and `_end_pass`, with `_open` noting the slot's file instead of opening it.  A subclass sets `self._slot_path = {}`
    before H5Loader's constructor runs and writes `plan_sample(batch)` -> a job tuple whose first entry is the path."""

    def _open(self, batch, path):  # (H5Loader opens the slot's file here; a plan only notes which one it is)
        self._slot_path[batch] = path

    def slot_flags(self, batch):
        return sum(bit for mech, bit in FLAG_BITS if self._flipped(mech, batch))

    def _restart(self, batch):
        """The slot moves on to the next file (h5.py:270-279); `reset_sequence` draws from np.random, so the order counts."""
        self._restarted = True
        if not self._threaded:
            self.new_seq = True
        self.reset_sequence(batch)
        self.batch_row[batch] = 0
        self.batch_idx[batch] = max(self.batch_idx) + 1
        self._open(batch, self.files[self.batch_idx[batch] % len(self.files)])

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

    def _delivered(self, restarted, done):
        """`H5Loader._deliver`'s bookkeeping for one planned batch handed on."""
        self.new_seq, self.pass_done = restarted, done
        self.samples += self.batch_size


class ResidentArena:
    """The device half of both loaders, mixed in FRONT of the plan: one arena per column over all files (`xs`, `ys` uint16, `ts`
    float64 relative to its file's t0, `ps` uint8 -- 13 bytes per event), int64 offsets, the hot-pixel statistics.  The loader
    gives `_produce(jobs, restarted, done)` -> a batch dict and keeps `self.last_row`, the (path, event index) of the last
    event handed out."""

    def _place(self, lengths):
        """Where every file's events start in the arena (host work: path -> events, in file order)."""
        self.offsets, at = {}, 0
        for path in self.files:
            self.offsets[path] = at
            at += lengths[path]
        self.total_events = at

    def _upload(self, cols):
        """The four columns (a list of per-file arrays each) and the statistics tensors; `resident_bytes`: the columns'."""
        dev = self.device
        self._xs, self._ys, self._ts, self._ps = (torch.from_numpy(np.concatenate(c)).to(dev) for c in cols)
        self.resident_bytes = sum(t.numel() * t.element_size() for t in (self._xs, self._ys, self._ts, self._ps))
        self.hot = bool(self.config["hot_filter"]["enabled"])
        if self.hot:
            self._hot_events = torch.zeros((self.batch_size, *self.res), dtype=torch.int32, device=dev)
            self._hot_obvs = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)

    def _hot_params(self):
        """evf_hot_pixels' (max_px, min_obvs, max_rate)."""
        hf = self.config["hot_filter"]
        return int(hf["max_px"]), int(hf["min_obvs"]), float(hf["max_rate"])

    def _mask_batch(self, out, mask):
        """The hot-pixel mask [B,H,W] applied in place to the three images of a batch dict."""
        for key, C in (("event_voxel", self.num_bins), ("event_cnt", 2), ("event_mask", 1)):
            _lib.call("evf_apply_pixel_mask", _lib.ptr(out[key]), _lib.ptr(mask), self.batch_size, C, *self.res)

    def __iter__(self):
        """The batches of one pass over the files, like `H5Loader.__iter__` with its flags: no reader thread, no device
        synchronisation."""
        try:
            for jobs, (restarted, done) in self.plan_batches():
                batch = self._produce(jobs, restarted, done)
                self._delivered(restarted, done)
                yield batch
        finally:
            self._end_pass()

    @property
    def last_proc_timestamp(self):
        """Timestamp (relative to its file's t0) of the last event handed out: fetched from the arena when asked for."""
        if self.last_row is not None:
            path, row = self.last_row
            self._last_ts = float(self._ts[self.offsets[path] + row])
            self.last_row = None
        return self._last_ts

    @last_proc_timestamp.setter
    def last_proc_timestamp(self, value):
        self.last_row, self._last_ts = None, value
