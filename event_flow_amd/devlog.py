"""What the device logs share on the host (monitor.TrainMonitor, activity.ActivityLog): a captured step appends one row to a
preallocated device tensor by plain launches (the conventions of csrc/evf_log.h) and names the row by ONE int64 word in device
memory -- the log's own word for eager steps, a word of a stepper's job table under the replayed steppers; nothing is read on the
host until `drain()`.

    Ring        step s goes to row s % rows; the owner drains before the ring wraps
    DeviceLog   the tensor, the row word and the drain behind a Ring
    append_csv  drained rows as a CSV file: the header when it is created, then appended to

`on_fused_engine` is the one answer to "do this network's spike words exist" that the logs and the evaluation steppers ask."""

import csv
import os

import torch

from . import _lib


def on_fused_engine(model):
    """(the network runs on the fused FireNet engine, the reason `model.compute_path` gives); the reason is None for a network
    that reports no compute path (none of the FireNet family).  Host only."""
    cp = getattr(model, "compute_path", None)
    if cp is None:
        return False, None
    return cp[0] == "fused", cp[1]


class Ring:
    """The ring rule of a device log of `rows` rows: pass s goes to row s % rows, and the owner drains before the ring wraps.
    Host arithmetic only."""

    def __init__(self, rows, what="ActivityLog"):
        self.rows, self.what = int(rows), what
        if self.rows < 1:
            raise _lib.EvflowError(f"{what}: a log of at least one row")
        self.steps, self.drained = 0, 0

    @property
    def pending(self):
        return self.steps - self.drained

    @property
    def full(self):
        """The next pass would overwrite an undrained row."""
        return self.pending >= self.rows

    def next_row(self, ahead=1):
        """The row the next pass fills.  Raises when the next `ahead` passes would reach a row that was not drained."""
        if self.pending + ahead > self.rows:
            raise _lib.EvflowError(f"{self.what}: {self.pending} undrained passes in a log of {self.rows} rows; call drain() before "
                                   "the ring wraps")
        return self.steps % self.rows

    def advance(self, n=1):
        self.steps += int(n)

    def take(self):
        """The rows written since the last drain, in pass order; they count as drained."""
        if self.pending > self.rows:
            raise _lib.EvflowError(f"{self.what}: {self.pending} passes since the last drain overwrote a log of {self.rows} rows")
        idx = [s % self.rows for s in range(self.drained, self.steps)]
        self.drained = self.steps
        return idx


class DeviceLog:
    """A ring of `rows` rows of `row_shape` elements on `device`, every element `fill` until a launch writes it, and the int64
    word that names the row of the next launch.  `log` is None until `allocate(row_shape, device)`: the constructor calls it when
    it is given the shape, an owner that learns the shape with its first row calls it then.

        log.use_row_word(ptr)       # the word of a stepper's job table; the stepper moves the ring (next_row / advance)
        log.begin()                 # else: the log's own word names ring.next_row() ...
        launch(..., log.row_ptr(), log.rows, _lib.ptr(log.log), ...)
        log.end()                   # ... and the ring moves on
    """

    def __init__(self, rows, row_shape=None, dtype=torch.float32, fill=0, device=None, what="DeviceLog"):
        self.ring = Ring(rows, what)
        self.rows, self.dtype, self.fill = self.ring.rows, dtype, fill
        self.log = self._row = self._ext = None
        if row_shape is not None:
            self.allocate(row_shape, device)

    def allocate(self, row_shape, device):
        self.log = torch.full((self.rows,) + tuple(row_shape), self.fill, dtype=self.dtype, device=device)
        self._row = torch.zeros(1, dtype=torch.int64, device=device)

    def use_row_word(self, ptr):
        """The row of every following launch is read from the int64 word at device address `ptr`, written by the caller, who
        also moves the ring; None: back to the log's own word."""
        self._ext = ptr

    def row_ptr(self):
        return self._ext if self._ext is not None else _lib.ptr(self._row)

    def begin(self):
        if self._ext is None:
            self._row.fill_(self.ring.next_row())

    def end(self, n=1):
        if self._ext is None:
            self.ring.advance(n)

    def drain(self):
        """The rows written since the last drain, in order, as a numpy array (None: there are none): one stream synchronise and
        one device -> host copy."""
        idx = self.ring.take()
        if not idx or self.log is None:
            return None
        if self.log.is_cuda:
            torch.cuda.current_stream().synchronize()
        return self.log.cpu().numpy()[idx]


def append_csv(path, header, lines):
    """Append `lines` to the CSV file `path`; it gets `header` when it is created."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a", newline="") as f:
        w = csv.writer(f)
        if new:
            w.writerow(header)
        w.writerows(lines)
