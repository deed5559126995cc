"""devlog.DeviceLog without a device (a log on the CPU; drain() synchronises only a CUDA log): the ring under an owner whose row
word is a stepper's (train.ResidentWindowStep: next_row() and advance() by the caller, begin() / end() never move the ring) and
under an owner with the log's own word, the drained rows in order across a wrap, the lazy allocation and the three messages."""

import ctypes

import numpy as np
import pytest
import torch

from event_flow_amd import _lib
from event_flow_amd.devlog import DeviceLog, append_csv


def _launch(log, value):
    """What a launch does: the row word at row_ptr() is read, and that row of the log written."""
    row = ctypes.c_int64.from_address(log.row_ptr()).value
    assert 0 <= row < log.rows
    log.log[row] = value


def test_own_row_word():
    log = DeviceLog(4, (2,), torch.float32, float("nan"), "cpu", "OwnLog")
    assert log.rows == 4 and tuple(log.log.shape) == (4, 2) and log.log.dtype == torch.float32 and bool(log.log.isnan().all())
    assert log.ring.pending == 0 and not log.ring.full and log.drain() is None
    for s in range(4):
        log.begin()
        _launch(log, s)
        log.end()
    assert log.ring.pending == 4 and log.ring.full and log.ring.steps == 4
    with pytest.raises(_lib.EvflowError, match="OwnLog.*drain"):
        log.begin()
    rows = log.drain()
    assert rows.dtype == np.float32 and rows.tolist() == [[s, s] for s in range(4)] and log.ring.pending == 0
    for s in range(4, 7):  # across the wrap: steps 4, 5, 6 fill rows 0, 1, 2
        log.begin()
        _launch(log, s)
        log.end()
    assert log.log[:, 0].tolist() == [4.0, 5.0, 6.0, 3.0] and log.drain().tolist() == [[4, 4], [5, 5], [6, 6]]
    for s in range(7, 10):  # rows 3, 0, 1
        log.begin()
        _launch(log, s)
        log.end()
    assert log.drain()[:, 0].tolist() == [7.0, 8.0, 9.0] and log.drain() is None
    log.begin()
    log.end(3)  # one launch that wrote three rows' worth of steps
    assert log.ring.pending == 3 and log.ring.steps == 13


def test_row_word_of_a_stepper():
    log = DeviceLog(3, (1,), torch.int32, -1, "cpu", "StepLog")
    table = torch.zeros(4, dtype=torch.int64)  # the stepper's job table; its last word names the row
    own = log.row_ptr()
    log.use_row_word(table.data_ptr() + 8 * 3)
    assert log.row_ptr() == table.data_ptr() + 24 != own
    for s in range(3):
        table[3] = log.ring.next_row()  # the caller's
        log.begin()
        _launch(log, 10 + s)
        log.end()
        assert log.ring.steps == s  # begin() / end() never move the ring under a caller's word
        log.ring.advance()  # the caller's
    assert log.ring.full and log.ring.pending == 3
    with pytest.raises(_lib.EvflowError, match="StepLog.*drain"):
        log.ring.next_row()
    log.begin()  # ... and never ask it either
    log.end()
    assert log.drain()[:, 0].tolist() == [10, 11, 12]
    table[3] = log.ring.next_row()
    _launch(log, 13)
    log.ring.advance()
    table[3] = -1  # a row word of -1 skips the launch; the step still counts
    log.ring.advance()
    assert log.drain()[:, 0].tolist() == [13, 11]
    log.ring.advance(4)
    with pytest.raises(_lib.EvflowError, match="StepLog.*overwrote"):
        log.drain()
    log.use_row_word(None)
    assert log.row_ptr() == own


def test_lazy_allocation_and_messages():
    log = DeviceLog(2, None, torch.int32, -1, what="LazyLog")
    assert log.log is None and log.rows == 2 and log.drain() is None
    log.allocate((3, 2), "cpu")
    assert tuple(log.log.shape) == (2, 3, 2) and log.log.dtype == torch.int32 and bool((log.log == -1).all())
    log.begin()
    _launch(log, 5)
    log.end()
    assert log.drain().shape == (1, 3, 2)
    with pytest.raises(_lib.EvflowError, match="LazyLog: a log of at least one row"):
        DeviceLog(0, (1,), device="cpu", what="LazyLog")


def test_append_csv_header_once(tmp_path):
    path = str(tmp_path / "deep" / "x.csv")
    append_csv(path, ["a", "b"], [[1, 2]])
    append_csv(path, ["a", "b"], [[3, 4], [5, 6]])
    with open(path, "rb") as f:
        assert f.read() == b"a,b\r\n1,2\r\n3,4\r\n5,6\r\n"
