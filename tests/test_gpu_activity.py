"""The activity log on the MI355X (csrc/evf_activity.hip, activity.ActivityLog, eval_flow.py --activity): the C ABI against
tests/activity_ref.py with exact integer counts -- every size, alignment, kind and special value, the row word between canary
rows, a captured call that follows its row word and its sources, every guard --, the log against `model(..., log=True)` on a
second model bit for bit, the evaluation's numbers untouched by an attached log, the replayed steppers against the same
launches run eagerly, and the driver on H5Loader, --resident and --resident --graphed: byte-identical activity.csv files."""

import copy
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

import activity_ref as ref
from test_gpu_deterministic import LIF_NEURON, G, _model_cfg
from test_gpu_eval_graphed import NAMES, SCALING as WIN_SCALING, _initial, det_on  # noqa: F401  (det_on: fixture)
from test_gpu_eval_graphed_aee import SCALING as AEE_SCALING, _capacity, _loader as _aee_loader, two_files
from test_gpu_head_det import PLIF_NEURON
from test_host_eval_steps import B as WB, H as WH, LENGTHS, N as WN, SEED, W as WW
from test_host_loader import _cfg
from test_host_resident import FLIPS, three_files

from event_flow_amd import _lib, synthetic
from event_flow_amd import activity as A
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.dataloader.resident import ResidentLoader
from event_flow_amd.evaluate import ResidentAEEStep, ResidentEvalStep
from event_flow_amd.loss.flow import FWL, RSAT
from event_flow_amd.models.model import LIFFireNet, PLIFFireNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
CANARY = 0x5A5A5A5A
NETS = {"lif": (LIFFireNet, LIF_NEURON), "plif": (PLIFFireNet, PLIF_NEURON)}


# ------------------------------------------------------------------ the C ABI
def _dev(arr, off):
    """uint32 / float32 host array [B, n] -> (its device copy at element offset `off` of a 16-byte aligned allocation whose other
    words are all ones -- a read outside the source would be counted --, the allocation)."""
    words = np.ascontiguousarray(arr).view(np.uint32).reshape(-1)
    full = torch.full((off + words.size + 7,), -1, dtype=torch.int32, device=DEV)
    assert full.data_ptr() % 16 == 0
    view = full[off:off + words.size]
    view.copy_(torch.from_numpy(words.view(np.int32).copy()))
    return view, full


class Call:
    """One evf_activity_at call: sources [(kind, host array [B, n], offset)], a log of `nrows` rows between two canary rows."""

    def __init__(self, sources, B, nrows=3):
        self.B, self.nrows, self.nsrc = B, nrows, len(sources)
        self.kinds = [k for k, _a, _o in sources]
        self.n = [a.shape[1] for _k, a, _o in sources]
        self.views = [_dev(a, off) for _k, a, off in sources]
        self.parts = int(_lib.load().evf_activity_parts(max(self.n)))
        assert self.parts >= 1
        self.row_words = self.nsrc * B * self.parts
        self.full = torch.full(((nrows + 2) * self.row_words,), 0, dtype=torch.int32, device=DEV)
        self.fill(CANARY)
        self.log = self.full[self.row_words:(nrows + 1) * self.row_words]
        self.row = torch.zeros(1, dtype=torch.int64, device=DEV)

    def fill(self, word):
        self.full.copy_(torch.from_numpy(np.full(self.full.numel(), word, dtype=np.uint32).view(np.int32)))

    def args(self, row_mul=1, row_add=0):
        return [(ctypes.c_void_p * self.nsrc)(*[v.data_ptr() for v, _f in self.views]), (ctypes.c_int * self.nsrc)(*self.kinds),
                (ctypes.c_int64 * self.nsrc)(*self.n), self.nsrc, self.B, self.row.data_ptr(), row_mul, row_add, self.nrows,
                self.log.data_ptr()]

    def run(self, row, row_mul=1, row_add=0):
        self.row.fill_(row)
        rc = _lib.raw("evf_activity_at", *self.args(row_mul, row_add))
        torch.cuda.synchronize()
        return rc

    def rows(self):
        """uint32 [nrows + 2][nsrc][B][parts]: the canary rows first and last."""
        return self.full.cpu().numpy().view(np.uint32).reshape(self.nrows + 2, self.nsrc, self.B, self.parts)

    def counts(self, r):
        return self.rows()[r + 1].astype(np.int64).sum(axis=2)

    def untouched(self, but=()):
        rows = self.rows()
        return all((rows[r + 1] == CANARY).all() for r in range(-1, self.nrows + 1) if r not in but)


def _want(sources):
    return ref.counts([(k, a) for k, a, _o in sources])


def _all_sources(B=3):
    """Every size x every element offset 0..3 x both kinds: 88 sources, the two kinds alternating."""
    rng = np.random.default_rng(11)
    out = []
    for n in ref.SIZES:
        for off in range(4):
            for kind in ((ref.FLOAT, ref.WORDS) if off % 2 == 0 else (ref.WORDS, ref.FLOAT)):
                data = ref.float_data(rng, B, n) if kind == ref.FLOAT else ref.word_data(rng, B, n)
                out.append((kind, data, off))
    return out


def test_counts_are_exact_for_every_size_offset_and_kind():
    """B = 3, every n of SIZES at element offsets 0, 1, 2 and 3, float data with both zeros, NaN, the infinities and the
    denormals, words with 0, 0xFFFFFFFF, 0x80000000 and 1; sixteen sources of both kinds and of different sizes a call."""
    sources = _all_sources()
    assert len(sources) == 88 and {(a.shape[1], o, k) for k, a, o in sources} == {(n, o, k) for n in ref.SIZES for o in range(4) for k in (0, 1)}
    sixteen = 0
    for lo in range(0, len(sources), 16):
        part = sources[lo:lo + 16]
        sixteen += len(part) == 16
        assert {k for k, _a, _o in part} == {ref.FLOAT, ref.WORDS}
        c = Call(part, 3)
        assert c.run(1) == 0
        got, want = c.counts(1), _want(part)
        assert got.shape == want.shape == (len(part), 3)
        assert np.array_equal(got, want), [(part[i][1].shape[1], part[i][2], part[i][0], got[i], want[i]) for i in range(len(part))
                                           if not np.array_equal(got[i], want[i])]
        assert c.untouched(but=(1,))
    assert sixteen == 5
    zero_f = [k for k, a, _o in sources if k == ref.FLOAT and (a.view(np.uint32) == 0x80000000).any() and np.isnan(a).any()]
    assert len(zero_f) >= 30  # (-0.0 and NaN are in the float sources from n = 3 on)


@pytest.mark.parametrize("n", [8193, 16389, 524295, 600001])
def test_counts_are_exact_across_parts(n):
    """Sizes at which a source is cut into parts (one more than a whole chunk, an uneven last share, more chunks than the most
    parts), beside a source of five elements whose later parts are empty."""
    rng = np.random.default_rng(n)
    parts = int(_lib.load().evf_activity_parts(n))
    assert parts >= 1
    sources = [(ref.FLOAT, ref.float_data(rng, 3, n), 1), (ref.WORDS, ref.word_data(rng, 3, n), 3), (ref.WORDS, ref.word_data(rng, 3, 5), 2),
               (ref.FLOAT, ref.float_data(rng, 3, n - 3), 0), (ref.FLOAT, ref.float_data(rng, 3, 5), 3)]
    c = Call(sources, 3)
    assert c.parts == parts
    c.fill(0xFFFFFFFF)  # every word of the addressed row is written
    assert c.run(0) == 0
    assert np.array_equal(c.counts(0), _want(sources))
    rows = c.rows()
    assert (rows[1] != 0xFFFFFFFF).all() and (rows[0] == 0xFFFFFFFF).all() and (rows[2:] == 0xFFFFFFFF).all()
    assert (rows[1][2, :, 2:] == 0).all()  # the empty shares of the five-word source store 0


def test_all_zero_and_all_ones():
    n = 1025
    zeros, ones = np.zeros((3, n), np.uint32), np.full((3, n), 0xFFFFFFFF, np.uint32)
    negz = np.full((3, n), -0.0, np.float32)
    sources = [(ref.WORDS, zeros, 1), (ref.WORDS, ones, 2), (ref.FLOAT, zeros.view(np.float32), 3), (ref.FLOAT, negz, 1),
               (ref.FLOAT, ones.view(np.float32), 0), (ref.FLOAT, np.full((3, n), 1e-45, np.float32), 2)]
    c = Call(sources, 3)
    assert c.run(2) == 0
    assert c.counts(2).tolist() == [[0] * 3, [32 * n] * 3, [0] * 3, [0] * 3, [n] * 3, [n] * 3]


def test_the_row_word():
    rng = np.random.default_rng(3)
    sources = [(ref.FLOAT, ref.float_data(rng, 3, 1023), 1), (ref.WORDS, ref.word_data(rng, 3, 1025), 2)]
    want = _want(sources)
    c = Call(sources, 3, nrows=7)
    for row in (-1, 7, 8, -2 ** 62, 2 ** 62, 2 ** 63 - 1, -2 ** 63):  # outside 0 .. nrows - 1: a defined no-op
        assert c.run(row) == 0 and c.untouched(), row
        assert c.run(row, 3, 2) == 0 and c.untouched(), row
    for row, mul, add in ((0, 1, 0), (6, 1, 0), (1, 3, 2), (2, 3, 0), (0, 3, 1), (5, 0, 4), (0, 0, 6), (-1, 0, 3), (2 ** 40, 0, 2)):
        at = A.pass_row(row, mul, add) if add < mul else row * mul + add  # the row computed on the host
        c.fill(0xFFFFFFFF if at % 2 else CANARY)
        assert c.run(row, mul, add) == 0
        rows = c.rows()
        filler = 0xFFFFFFFF if at % 2 else CANARY
        assert np.array_equal(rows[at + 1].astype(np.int64).sum(axis=2), want), (row, mul, add)
        assert (rows[at + 1] != filler).all()  # every word of the addressed row is written
        assert all((rows[r] == filler).all() for r in range(9) if r != at + 1), (row, mul, add)  # its neighbours bit-identical
    for row, mul, add in ((2, 3, 1), (1, 3, 4), (7, 1, 0), (-1, 3, 2), (3, 2 ** 62, 0), (1, 2 ** 63 - 1, 2 ** 63 - 1)):  # 7, 7, 7, -1, 3 * 2^62
        c.fill(CANARY)
        assert c.run(row, mul, add) == 0 and c.untouched(), (row, mul, add)


def test_a_captured_call_follows_the_row_word_and_the_sources():
    rng = np.random.default_rng(8)
    sources = [(ref.FLOAT, ref.float_data(rng, 3, 4099), 3), (ref.WORDS, ref.word_data(rng, 3, 1024), 1)]
    c = Call(sources, 3, nrows=6)
    assert c.run(0, 2, 1) == 0 and np.array_equal(c.counts(1), _want(sources))  # (not captured: the kernel is loaded)
    c.fill(CANARY)
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        assert _lib.raw("evf_activity_at", *c.args(2, 1)) == 0
    torch.cuda.synchronize()
    assert c.untouched()  # captured, not run
    wants = {}
    for k, row in enumerate((2, 0, 1)):  # rows 5, 1, 3
        data = [ref.float_data(rng, 3, 4099, zeros=0.2 + 0.3 * k), ref.word_data(rng, 3, 1024) & np.uint32(0xFFFF << (8 * k))]
        for (view, _full), a in zip(c.views, data):
            view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()))
        c.row.fill_(row)
        g.replay()
        torch.cuda.synchronize()
        wants[2 * row + 1] = ref.counts([(ref.FLOAT, data[0]), (ref.WORDS, data[1])])
    assert len({w.tobytes() for w in wants.values()}) == 3
    for at, want in wants.items():
        assert np.array_equal(c.counts(at), want), at
    assert c.untouched(but=tuple(wants))


def test_host_guards():
    rng = np.random.default_rng(2)
    sources = [(k % 2, ref.word_data(rng, 2, 8 + k) if k % 2 else ref.float_data(rng, 2, 8 + k), k % 4) for k in range(16)]
    c = Call(sources, 2)
    ok = c.args(3, 2)  # src, kind, n, nsrc, B, row, row_mul, row_add, nrows, log
    bad = [(k, None) for k in (0, 1, 2, 5, 9)]                                     # null pointers
    bad += [(3, v) for v in (0, -1, 17)] + [(4, v) for v in (0, -1, 65536)]       # nsrc outside 1..16; B
    bad += [(8, 0), (8, -1), (6, -1), (7, -1), (6, -2 ** 63), (7, -2 ** 63)]       # nrows; negative row_mul / row_add
    bad += [(9, ok[9] + 2), (5, ok[5] + 4)]                                        # misaligned log and row word
    for at, value in bad:
        args = list(ok)
        args[at] = value
        assert _lib.raw("evf_activity_at", *args) == EINVAL, (at, value)

    def with_entry(which, k, value):
        args = list(ok)
        vals = {0: [v.data_ptr() for v, _f in c.views], 1: list(c.kinds), 2: list(c.n)}[which]
        vals[k] = value
        args[which] = {0: ctypes.c_void_p * 16, 1: ctypes.c_int * 16, 2: ctypes.c_int64 * 16}[which](*vals)
        return args

    for k in (0, 15):
        assert _lib.raw("evf_activity_at", *with_entry(0, k, None)) == EINVAL       # a null source
        assert _lib.raw("evf_activity_at", *with_entry(0, k, c.views[k][0].data_ptr() + 2)) == EINVAL  # a misaligned one
        for kind in (-1, 2, 7):
            assert _lib.raw("evf_activity_at", *with_entry(1, k, kind)) == EINVAL
        for n in (0, -1, 2 ** 27, 2 ** 31, 2 ** 32 + 8, -2 ** 63):
            assert _lib.raw("evf_activity_at", *with_entry(2, k, n)) == EINVAL, n
    lib = _lib.load()
    assert [int(lib.evf_activity_parts(v)) for v in (0, -1, 2 ** 27, 2 ** 40)] == [EINVAL] * 4
    assert int(lib.evf_activity_parts(2 ** 27 - 1)) >= 1 and int(lib.evf_activity_parts(1)) >= 1
    torch.cuda.synchronize()
    assert c.untouched()  # no refused call stored anything
    assert c.run(0, 3, 2) == 0 and np.array_equal(c.counts(2), _want(sources))


# ------------------------------------------------------------------ ActivityLog against model(..., log=True)
def _start(kind):
    """test_gpu_train_monitor._start: an alive network (seed 3, thresholds x 0.25) -> its state_dict.  On the CPU oracle this
    recipe leaves every spiking layer between 25 % and 57 % active at both shapes used below."""
    cls, neuron = NETS[kind]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh"):
                p.mul_(0.25)
    return copy.deepcopy(first.state_dict())


def _model(kind, sd0):
    cls, neuron = NETS[kind]
    m = cls(_model_cfg(neuron)).to(DEV)
    m.load_state_dict(sd0)
    m.eval()
    assert m.compute_path[0] == "fused", m.compute_path
    return m


def _cnt(B, n, H, W, seed):
    return encode_event_list(G(synthetic.event_list_batch(B, n, H, W, seed)), 2, (H, W), want=("cnt",))["event_cnt"]


@pytest.mark.parametrize("kind", sorted(NETS))
def test_the_log_is_log_true_bit_for_bit(kind):
    B, H, W, n = 2, 32, 32, 400
    sd0 = _start(kind)
    m, twin = _model(kind, sd0), _model(kind, sd0)
    log = A.ActivityLog(m, B, rows=8)
    want, flows = [], []
    with torch.no_grad():
        for k in range(6):
            if k == 3:
                m.reset_states()
                twin.reset_states()
            x = _cnt(B, n, H, W, 9100 + k)
            flow = m(None, x)["flow"][-1]
            log.record(*m.last_io())
            out = twin(None, x, log=True)
            assert torch.equal(flow, out["flow"][-1])
            want.append([out["activity"][layer] for layer in A.LAYERS])
    assert log.pending == 6
    counts = log.drain()
    assert counts.shape == (6, 9, B) and counts.dtype == np.int64 and log.pending == 0 and log.drain().shape == (0, 9, B)
    batch, slots = log.fractions(counts)
    bits = np.array(A.layer_bits(2, H, W))
    assert all(b & (b - 1) == 0 and B * b < 2 ** 24 for b in bits)  # powers of two below 2^24: the float32 mean is exact
    print(kind, "batch-wide fractions", batch.tolist())
    got32, want32 = batch.astype(np.float32), np.array(want, dtype=np.float32)
    assert np.array_equal(got32.astype(np.float64), batch)  # (exact in float32)
    assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32)), (got32, want32)
    partial = ((counts > 0) & (counts < bits[None, :, None])).any(axis=(0, 2))  # per layer: 0 < count < bits in some pass
    assert partial[1] and int(partial[1:8].sum()) >= 5, partial  # 1:head and at least four more of the seven spiking layers
    assert not np.array_equal(counts[2], counts[3])
    log.close()


@pytest.mark.parametrize("kind", sorted(NETS))
def test_the_log_counts_its_sources(kind):
    """24 x 40, B = 3 (no power of two): integers against count_nonzero and a popcount of clones of x, the spike words and the
    flow; a ring of four rows that wraps."""
    B, H, W, n = 3, 24, 40, 400
    m = _model(kind, _start(kind))
    log = A.ActivityLog(m, B, rows=4)
    want, got = [], []
    with torch.no_grad():
        for k in range(6):
            if k == 3:
                m.reset_states()
            if log.full:
                got.append(log.drain())
            m(None, _cnt(B, n, H, W, 9200 + k))
            log.record(*m.last_io())
            x, flow = m.last_io()
            words = [st[1].clone() for st in m.state_buffers()]
            want.append(ref.counts([(ref.FLOAT, x.cpu().numpy().reshape(B, -1))] + [(ref.WORDS, z.cpu().numpy().reshape(B, -1)) for z in words]
                                   + [(ref.FLOAT, flow.cpu().numpy().reshape(B, -1))]))
    got.append(log.drain())
    assert [g.shape[0] for g in got] == [4, 2]
    got, want = np.concatenate(got), np.stack(want)
    assert np.array_equal(got, want)
    bits = np.array(A.layer_bits(2, H, W))
    assert ((got[:, 1:8] > 0) & (got[:, 1:8] < bits[None, 1:8, None])).all() and (got[:, 0] > 0).all() and (got[:, 8] > 0).all()
    with pytest.raises(_lib.EvflowError, match="built for"):
        log.record(torch.zeros(2, 2, H, W, device=DEV), torch.zeros(2, 2, H, W, device=DEV))
    log.close()
    with pytest.raises(RuntimeError, match="keep_io"):
        m.last_io()


# ------------------------------------------------------------------ the steppers: nothing changes, replay == eager
def _run_windows(path, sd0, replay, P, logged):
    model = _model("lif", sd0)
    config = {"loader": {"resolution": [WH, WW]}, "loss": {"overwrite_intermediate": False}}
    criteria = [FWL(config, DEV, flow_scaling=WIN_SCALING), RSAT(config, DEV, flow_scaling=WIN_SCALING)]
    np.random.seed(SEED)
    random.seed(SEED)
    ld = ResidentLoader(_cfg(path, "events", WN, WB, (WH, WW), FLIPS, hot=True), 2)
    steps = list(ld.plan_eval_steps(P))
    passes = sum(len(g) for g, _r, _t in steps)
    log = A.ActivityLog(model, WB, rows=passes) if logged else None
    stepper = ResidentEvalStep(model, criteria, NAMES, ld, P, len(steps) - 1, WIN_SCALING, warmup=2, replay=replay, per_sequence=True,
                               activity=log)
    for group, pass_reset, tail in steps:
        stepper.step_tail(group, pass_reset) if tail else stepper.step(group, pass_reset)
    counts = None
    if logged:
        torch.cuda.current_stream().wait_stream(stepper.stream)
        torch.cuda.synchronize()
        raw = log.log.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=3)
        assert log.pending == passes
        counts = raw[:passes]
    out = stepper.results()
    torch.cuda.synchronize()
    tail = torch.stack(stepper.tail_sharp) if stepper.tail_sharp else torch.empty(0, device=DEV)
    new = [bool(r) for _g, rs, _t in steps for r in rs]
    return dict(log=stepper.log.clone(), tail=tail.clone(), out=out, states=[s.clone() for s in model.states], counts=counts,
                stats=dict(stepper.stats), new=new, pass_new=list(stepper.pass_new), files=stepper.pass_files, passes=passes)


def test_window_stepper_replayed_logs_are_the_eager_logs_and_change_nothing(tmp_path, det_on):  # noqa: F811
    three_files(tmp_path, H=WH, W=WW, lengths=LENGTHS)
    sd0 = _initial("lif")
    P = 3
    r, e, bare = (_run_windows(tmp_path, sd0, True, P, True), _run_windows(tmp_path, sd0, False, P, True),
                  _run_windows(tmp_path, sd0, True, P, False))
    assert r["passes"] == 35 and r["stats"]["replayed"] == 35 // P - 2 and r["stats"]["tail_passes"] == 35 % P == 2 and e["stats"]["replayed"] == 0
    assert any(not rs[0] and any(rs[1:]) for rs in [r["new"][i:i + P] for i in range(0, 33, P)][2:])  # a restart inside a replayed window
    assert r["counts"].shape == (35, 9, WB) and np.array_equal(r["counts"], e["counts"])  # rows == forwards of the loop
    bits = np.array(A.layer_bits(2, WH, WW))
    assert ((r["counts"] <= bits[None, :, None]).all() and (r["counts"][:, 1:8].sum(axis=(1, 2)) > 0).all()
            and len({row.tobytes() for row in r["counts"]}) == 35)
    assert r["pass_new"] == e["pass_new"] == r["new"] and sum(r["new"]) >= 2
    assert r["files"] == e["files"] and len(r["files"]) == 35 and {f for row in r["files"] for f in row} == {"s0.npz", "s1.npz", "s2.npz"}
    assert r["out"] == e["out"] and set(r["out"]["activity"]) == set(A.LAYERS)
    assert all(set(v) >= {"activity"} for v in r["out"]["per_sequence"].values())
    # with the log attached, not one number of the evaluation changes
    assert torch.equal(r["log"], bare["log"]) and torch.equal(r["tail"], bare["tail"]) and r["stats"] == bare["stats"]
    assert all(torch.equal(a, b) for a, b in zip(r["states"], bare["states"]))
    assert bare["counts"] is None and "activity" not in bare["out"]
    assert {k: v for k, v in r["out"].items() if k not in ("activity", "per_sequence")} == {k: v for k, v in bare["out"].items() if k != "per_sequence"}
    for f, v in bare["out"]["per_sequence"].items():
        assert "activity" not in v and {k: x for k, x in r["out"]["per_sequence"][f].items() if k != "activity"} == v
    # "activity" is the mean over the passes of the batch-wide fraction
    batch, _slots = A.fractions(r["counts"], bits)
    for l, layer in enumerate(A.LAYERS):
        assert r["out"]["activity"][layer] == float(sum(batch[:, l]) / 35)


def _run_aee(path, sd0, mode, window, B, replay, logged):
    model = _model("lif", sd0)
    ld = _aee_loader(path, mode, window, B, True)
    plan = list(ld.plan_eval_passes())
    evals = sum(1 for _j, _r, e in plan if e)
    log = A.ActivityLog(model, B, rows=len(plan)) if logged else None
    stepper = ResidentAEEStep(model, ld, len(plan), evals, _capacity(plan), AEE_SCALING, warmup=2, replay=replay, per_sequence=True,
                              activity=log)
    model.reset_states()
    for jobs, restarted, evaluate in plan:
        stepper.step(jobs, restarted, evaluate)
    counts = None
    if logged:
        torch.cuda.current_stream().wait_stream(stepper.stream)
        torch.cuda.synchronize()
        counts = log.log.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=3)
    out = stepper.results()
    torch.cuda.synchronize()
    return dict(aee=stepper.aee_log.clone(), sharp=stepper.sharp_log.clone(), out=out, states=[s.clone() for s in model.states],
                counts=counts, stats=dict(stepper.stats), new=[bool(r) for _j, r, _e in plan], pass_new=list(stepper.pass_new),
                files=stepper.pass_files, passes=len(plan))


@pytest.mark.parametrize("mode,window", [("gtflow_dt1", 1), ("gtflow_dt4", 0.25)])
def test_aee_stepper_replayed_logs_are_the_eager_logs_and_change_nothing(tmp_path, det_on, mode, window):  # noqa: F811
    two_files(tmp_path)
    sd0 = _initial("lif")
    B = 2
    r, e, bare = (_run_aee(tmp_path, sd0, mode, window, B, True, True), _run_aee(tmp_path, sd0, mode, window, B, False, True),
                  _run_aee(tmp_path, sd0, mode, window, B, True, False))
    n = r["passes"]
    assert r["stats"]["replayed"] == n - 2 and r["stats"]["replayed_reset"] >= 1 and e["stats"]["replayed"] == 0
    assert r["counts"].shape == (n, 9, B) and np.array_equal(r["counts"], e["counts"])  # one row per forward of the loop
    assert (r["counts"][:, 1:8].sum(axis=(1, 2)) > 0).sum() >= n // 2  # (the first windows of a file hold no events)
    assert r["pass_new"] == e["pass_new"] == r["new"] and r["files"] == e["files"] and len(r["files"]) == n
    assert r["out"] == e["out"] and set(r["out"]["activity"]) == set(A.LAYERS)
    assert torch.equal(r["aee"], bare["aee"]) and torch.equal(r["sharp"], bare["sharp"]) and r["stats"] == bare["stats"]
    assert all(torch.equal(a, b) for a, b in zip(r["states"], bare["states"]))
    assert "activity" not in bare["out"]
    assert {k: v for k, v in r["out"].items() if k not in ("activity", "per_sequence")} == {k: v for k, v in bare["out"].items() if k != "per_sequence"}
    for f, v in bare["out"]["per_sequence"].items():
        assert {k: x for k, x in r["out"]["per_sequence"][f].items() if k != "activity"} == v


# ------------------------------------------------------------------ the driver
def _driver_files(tmp_path, mode, B, model=None, neuron=True):
    import eval_flow

    (tmp_path / "data").mkdir()
    root = os.path.dirname(os.path.abspath(eval_flow.__file__))
    tcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_SNN.yml")))
    tcfg["spiking_neuron"]["thresh"] = [0.2, 0.05]
    if model:
        tcfg["model"].update(model)
    if not neuron:
        del tcfg["spiking_neuron"]
    ecfg = yaml.safe_load(open(os.path.join(root, "configs", "eval_flow.yml")))
    if mode == "events":
        H, W = WH, WW
        three_files(tmp_path / "data", H=H, W=W, lengths=LENGTHS)
        ecfg["data"].update(path=str(tmp_path / "data"), mode="events", window=WN, window_eval=3 * WN)
        ecfg["metrics"]["name"] = list(NAMES)
    else:
        H, W = 32, 40
        two_files(tmp_path / "data")
        ecfg["data"].update(path=str(tmp_path / "data"), mode=mode, window=1, window_eval=1)
        ecfg["metrics"].update(name=["AEE"], flow_scaling=AEE_SCALING)
    tcfg["loader"].update(resolution=[H, W])
    ecfg["loader"].update(batch_size=B, resolution=[H, W], augment=list(FLIPS), augment_prob=[0.5, 0.5, 0.5])
    ecfg["hot_filter"] = {"enabled": True, "max_px": 100, "min_obvs": 2, "max_rate": 0.8}
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))


def _drive(tmp_path, capsys, seed, activity, resident=False, graphed=False, replay=True, per_sequence=True, vis=False):
    import eval_flow
    from event_flow_amd.configs.parser import YAMLParser

    torch.manual_seed(4)
    np.random.seed(seed)
    random.seed(seed)
    args = types.SimpleNamespace(train_config=str(tmp_path / "train.yml"), weights="", synthetic=False, sequences=4, resident=resident,
                                 store="", graphed=graphed, per_sequence=per_sequence)
    if activity is not None:
        args.activity = str(tmp_path / activity) if activity else ""
    parser = YAMLParser(str(tmp_path / "eval.yml"))
    if vis:
        parser.config.setdefault("vis", {})["activity"] = True
    capsys.readouterr()
    out = eval_flow.test(args, parser, graphed_replay=replay)
    captured = capsys.readouterr()
    assert json.loads(captured.out.strip().splitlines()[-1]) == out
    return out, captured.err


def _csv(tmp_path, name):
    return open(tmp_path / name / "activity.csv", "rb").read()


def test_driver_events_on_all_three_paths(tmp_path, det_on, capsys):  # noqa: F811
    _driver_files(tmp_path, "events", WB)
    (g1, _), (g0, _) = _drive(tmp_path, capsys, SEED, "g1", True, True), _drive(tmp_path, capsys, SEED, "g0", True, True, replay=False)
    (res, _), (h5, _) = _drive(tmp_path, capsys, SEED, "res", True), _drive(tmp_path, capsys, SEED, "h5")
    (off, _), (unset, _) = _drive(tmp_path, capsys, SEED, None), _drive(tmp_path, capsys, SEED, "")
    assert g1["graphed"]["replayed"] == 9 and g0["graphed"]["replayed"] == 0
    files = {name: _csv(tmp_path, name) for name in ("g1", "g0", "res", "h5")}
    assert files["g1"] == files["g0"] == files["res"] == files["h5"]
    lines = files["g1"].decode().split("\r\n")
    assert lines[0].split(",") == ["pass", "new_seq"] + list(A.LAYERS) + [f"b{k}/{layer}" for k in range(WB) for layer in A.LAYERS]
    assert len(lines) == 1 + 35 + 1 and [ln.split(",")[0] for ln in lines[1:-1]] == [str(k) for k in range(35)]  # a row per forward
    table = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:-1]])
    assert table[0, 1] == 1 and 3 <= table[:, 1].sum() < 35 and (table[:, 2] > 0).all() and (table[:, 2:] <= 1).all()
    assert (table[:, 3] > 0).any() and len({tuple(row[2:]) for row in table}) == 35
    for name, other in (("replay off", g0), ("--resident", res), ("H5Loader", h5)):
        assert g1["activity"] == other["activity"], name
        assert g1["per_sequence"] == other["per_sequence"], name
    assert set(g1["activity"]) == set(A.LAYERS)
    for l, layer in enumerate(A.LAYERS):
        assert abs(g1["activity"][layer] - table[:, 2 + l].mean()) <= 1e-6
    # per sequence: a slot's passes go to the file the plan says that slot reads in that pass
    np.random.seed(SEED)
    random.seed(SEED)
    ld = ResidentLoader(_cfg(tmp_path / "data", "events", WN, WB, (WH, WW), FLIPS, hot=True), 2)
    names = [[os.path.basename(job[0]) for job in jobs] for group, _r, _t in ld.plan_eval_steps(3) for jobs, _rs, _d in group]
    assert len(names) == 35 and any(row[0] != row[1] for row in names)
    sums = {}
    for k, row in enumerate(names):
        for b, f in enumerate(row):
            cell = sums.setdefault(f, [np.zeros(9), 0])
            cell[0] += table[k, 2 + 9 * (1 + b):2 + 9 * (2 + b)]
            cell[1] += 1
    assert set(sums) == set(g1["per_sequence"]) == {"s0.npz", "s1.npz", "s2.npz"} and len({n for _s, n in sums.values()}) >= 2
    for f, (s, n) in sums.items():
        assert set(g1["per_sequence"][f]) == {"FWL", "RSAT", "it", "activity"}
        for l, layer in enumerate(A.LAYERS):
            assert abs(g1["per_sequence"][f]["activity"][layer] - s[l] / n) <= 1e-6, (f, layer)
    # without the flag: no key, no file, and the flag changes no other number
    for name in (off, unset):
        assert "activity" not in name and all("activity" not in v for v in name["per_sequence"].values())
        assert {k: v for k, v in h5.items() if k not in ("activity", "per_sequence")} == {k: v for k, v in name.items() if k != "per_sequence"}
        for f, v in name["per_sequence"].items():
            assert {k: x for k, x in h5["per_sequence"][f].items() if k != "activity"} == v
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["data", "train.yml", "eval.yml", "g1", "g0", "res", "h5"])


def test_driver_aee_on_all_three_paths(tmp_path, det_on, capsys):  # noqa: F811
    _driver_files(tmp_path, "gtflow_dt1", 2)
    (g1, _), (res, _), (h5, _) = (_drive(tmp_path, capsys, 9, "g1", True, True), _drive(tmp_path, capsys, 9, "res", True),
                                  _drive(tmp_path, capsys, 9, "h5"))
    assert g1["graphed"]["replayed"] >= 3
    assert _csv(tmp_path, "g1") == _csv(tmp_path, "res") == _csv(tmp_path, "h5")
    assert len(_csv(tmp_path, "g1").decode().split("\r\n")) == 1 + g1["graphed"]["passes"] + 1
    assert g1["activity"] == res["activity"] == h5["activity"] and g1["activity"]["0:input"] > 0
    for f in ("seq0.npz", "seq1.npz"):
        assert g1["per_sequence"][f]["activity"] == res["per_sequence"][f]["activity"] == h5["per_sequence"][f]["activity"]


def test_driver_vis_activity_means_the_working_directory(tmp_path, det_on, capsys, monkeypatch):  # noqa: F811
    _driver_files(tmp_path, "events", 1)
    (tmp_path / "cwd").mkdir()
    monkeypatch.chdir(tmp_path / "cwd")
    out, _ = _drive(tmp_path, capsys, SEED, None, resident=True, per_sequence=False, vis=True)
    lines = open(tmp_path / "cwd" / "activity.csv", "rb").read().decode().split("\r\n")
    assert lines[0] == "pass,new_seq," + ",".join(A.LAYERS) and len(lines) > 10 and set(out["activity"]) == set(A.LAYERS)


def test_driver_general_path_falls_back_to_log_true(tmp_path, det_on, capsys):  # noqa: F811
    _driver_files(tmp_path, "events", WB, model={"base_num_channels": 16})
    out, err = _drive(tmp_path, capsys, SEED, "gen", resident=True, per_sequence=False)
    assert "general path" in err and "model(..., log=True)" in err
    lines = _csv(tmp_path, "gen").decode().split("\r\n")
    assert lines[0].split(",") == ["pass", "new_seq"] + list(A.LAYERS) + [f"b{k}/{layer}" for k in range(WB) for layer in A.LAYERS]
    assert len(lines) == 1 + 35 + 1 and all(len(ln.split(",")) == 2 + 9 * (1 + WB) for ln in lines[1:-1])
    table = np.array([[float(v) for v in ln.split(",")[:11]] for ln in lines[1:-1]])
    assert (table[:, 2] > 0).all() and (table[:, 2:] <= 1).all() and set(out["activity"]) == set(A.LAYERS)
    assert abs(out["activity"]["0:input"] - table[:, 2].mean()) <= 1e-6
    with pytest.raises(_lib.EvflowError, match="general path"):  # (--graphed refuses the general path as before)
        _drive(tmp_path, capsys, SEED, "gen2", resident=True, graphed=True, per_sequence=False)


def test_driver_refuses_an_evflownet(tmp_path, det_on, capsys):  # noqa: F811
    _driver_files(tmp_path, "events", WB, model={"name": "EVFlowNet", "base_num_channels": 8, "activations": ["relu", None]}, neuron=False)
    with pytest.raises(_lib.EvflowError, match='EVFlowNet.forward reports "activity": None'):
        _drive(tmp_path, capsys, SEED, "ev", per_sequence=False)
    assert not (tmp_path / "ev").exists()
