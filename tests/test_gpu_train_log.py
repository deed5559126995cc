"""The training log's kernels (csrc/evf_train_log.hip: evf_grad_stats_partial / _store, evf_spike_count, evf_spike_rates_store) on
the MI355X through the C ABI, against the float64 / numpy restatement of tests/train_log_ref.py: gradient statistics after
clipping (min and max bit-equal to torch's on a clone, mean within one float32 rounding), exact spike counts and rates, the
log discipline (a row word outside the log is a no-op, a valid one writes its payload only, two calls give the same bits),
captured calls replayed with changed inputs, and every EVF_EINVAL guard."""

import ctypes

import numpy as np
import pytest
import torch

import train_log_ref as ref
from gpu_bufs import Bufs

from event_flow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
EINVAL = -22
CANARY = 0x7FC12345  # a NaN no kernel produces
NROWS, OFFSET, SPARE = 4, 2, 3


def rc_of(name, *args):
    return getattr(_lib.load(), name)(*args, _lib.stream_ptr())


def canary_log(row_floats):
    return torch.full((NROWS * row_floats,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)


def log_bits(log):
    return log.view(torch.int32).cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- gradient statistics
class GradCase:
    """Nine segments of sizes around the block and the chunk, at offsets that are no multiples of 4 elements, in one guarded flat
    buffer; values: seeded normals with 0.0, -0.0, a denormal and negatives among them."""

    def __init__(self, seed=0):
        lib = _lib.load()
        self.chunk = chunk = int(lib.evf_grad_stats_chunk())
        self.sizes = [1, 3, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
        self.segs, off = [], 1
        for k, n in enumerate(self.sizes):
            while off % 4 != 1 + k % 3:  # 1, 2, 3, 1, ...: never 16-byte aligned
                off += 1
            self.segs.append((off, n))
            off += n + 2
        self.total_len = off
        rng = np.random.default_rng(seed)
        g = rng.standard_normal(self.total_len).astype(F32)
        for o, n in self.segs:
            if n >= 255:
                g[o + 5], g[o + 77], g[o + 130], g[o + n - 1] = 0.0, -0.0, 1e-40, -3.5
        self.g = g
        self.nseg, self.max_n = len(self.segs), max(self.sizes)
        self.payload = 3 + 3 * self.nseg
        self.row_floats = OFFSET + self.payload + SPARE
        self.bufs = Bufs()
        self.grad = self.bufs.new(g)
        self.ws_floats = int(lib.evf_grad_stats_ws(self.nseg, self.max_n))
        assert self.ws_floats == self.nseg * 3 * 5
        self.ws = self.bufs.new(np.zeros(self.ws_floats, F32), shift=1)
        self.seg_off = torch.tensor([o for o, _n in self.segs], dtype=torch.int64, device=DEV)
        self.seg_n = torch.tensor([n for _o, n in self.segs], dtype=torch.int64, device=DEV)
        self.norm_ws = torch.zeros(8, dtype=torch.float32, device=DEV)
        self.norm_src = torch.zeros(1, dtype=torch.float32, device=DEV)
        self.loss = torch.tensor([1.25], dtype=torch.float32, device=DEV)
        self.row = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.log = canary_log(self.row_floats)

    def partial(self):
        _lib.call("evf_grad_stats_partial", self.grad.ptr, _lib.ptr(self.seg_off), _lib.ptr(self.seg_n), self.nseg, self.max_n,
                  self.ws.ptr, self.ws_floats)

    def stand_in_step(self):
        """What the optimizer's step kernel does for the log: the squared norm into norm_ws[0] (an element-wise kernel)."""
        torch.mul(self.norm_src, 1.0, out=self.norm_ws[:1])

    def store(self, max_norm, loss=True):
        _lib.call("evf_grad_stats_store", self.ws.ptr, self.ws_floats, _lib.ptr(self.seg_n), self.nseg, self.max_n,
                  _lib.ptr(self.norm_ws), float(max_norm), _lib.ptr(self.loss) if loss else None, _lib.ptr(self.row), NROWS,
                  _lib.ptr(self.log), self.row_floats, OFFSET)

    def run(self, max_norm, loss=True):
        self.partial()
        self.stand_in_step()
        self.store(max_norm, loss)
        torch.cuda.synchronize()
        self.bufs.check()

    def set_total(self, total):
        self.norm_src.fill_(float(total))

    def payload_of(self, row):
        lo = row * self.row_floats + OFFSET
        return self.log.cpu().numpy()[lo:lo + self.payload].copy()

    def check_row(self, row, g, total, max_norm, loss=1.25):
        """The row against torch on a clone (min, max: bits), float64 (mean) and numpy float32 (norm, coef)."""
        got = self.payload_of(row)
        norm, coef = ref.clip_head(total, max_norm)
        assert ref.bits(got[1]) == ref.bits(norm) and ref.bits(got[2]) == ref.bits(coef), (got[1:3], norm, coef)
        if loss is not None:
            assert ref.bits(got[0]) == ref.bits(F32(loss))
        clone = torch.from_numpy(np.array(g, F32)).to(DEV)
        means = ref.grad_means(g, self.segs, coef)
        for k, (o, n) in enumerate(self.segs):
            scaled = (clone[o:o + n] * float(coef)).abs()
            mean, mn, mx = got[3 + 3 * k:6 + 3 * k]
            want_mn, want_mx = scaled.min().cpu().numpy(), scaled.max().cpu().numpy()
            print(f"segment {k} n={n}: mean {mean!r} (float64 {means[k]!r}) min {mn!r} / {want_mn!r} max {mx!r} / {want_mx!r}")
            assert ref.bits(mn) == ref.bits(want_mn) and ref.bits(mx) == ref.bits(want_mx), (k, mn, want_mn, mx, want_mx)
            assert abs(float(mean) - means[k]) <= ref.MEAN_RTOL * abs(means[k]), (k, mean, means[k])
        return got


@pytest.fixture(scope="module")
def grad_case():
    return GradCase()


@pytest.mark.parametrize("case", ["clipped", "unclipped", "no_clip"])
def test_grad_stats_after_clipping(grad_case, case):
    c = grad_case
    total = F32((c.g.astype(np.float64) ** 2).sum())  # (any positive float32 would do: the stand-in writes it)
    norm = float(np.sqrt(total))
    max_norm = {"clipped": 0.37 * norm, "unclipped": 100.0 * norm, "no_clip": 0.0}[case]
    c.set_total(total)
    c.row.fill_(2)
    c.run(max_norm)
    got = c.check_row(2, c.g, total, max_norm)
    assert (got[2] < 1) == (case == "clipped") and (case == "clipped" or got[2] == 1)
    assert min(got[4::3][2:]) == 0.0  # (the planted zeros are the minima of the segments that hold them)


def test_grad_stats_nan_and_inf(grad_case):
    c = grad_case
    total = F32(4.0)
    c.set_total(total)
    c.row.fill_(1)
    c.run(1.0)
    clean = c.payload_of(1)
    g = c.g.copy()
    g[c.segs[4][0] + 200] = np.nan
    g[c.segs[8][0] + c.chunk + 3] = -np.inf
    c.grad.set(g)
    try:
        c.run(1.0)
        got = c.payload_of(1)
    finally:
        c.grad.set(c.g)
    assert np.isnan(got[3 + 12:6 + 12]).all()
    mean, mn, mx = got[3 + 24:6 + 24]
    assert np.isposinf(mean) and np.isposinf(mx) and ref.bits(mn) == ref.bits(clean[4 + 24])
    keep = [i for i in range(c.payload) if not (15 <= i < 18 or 27 <= i < 30)]
    assert np.array_equal(ref.bits(got[keep]), ref.bits(clean[keep]))


def test_grad_stats_log_discipline(grad_case):
    c = grad_case
    c.set_total(9.0)
    c.log.copy_(canary_log(c.row_floats))
    for word in (-1, NROWS, 2 ** 40, -2 ** 40):
        c.row.fill_(word)
        c.run(1.0)
        assert (log_bits(c.log) == CANARY).all(), word
    c.row.fill_(3)
    c.run(1.0)
    first = log_bits(c.log)
    lo = 3 * c.row_floats + OFFSET
    inside = np.zeros(first.size, bool)
    inside[lo:lo + c.payload] = True
    assert (first[~inside] == CANARY).all() and (first[inside] != CANARY).all()
    c.run(1.0)
    assert np.array_equal(log_bits(c.log), first)
    # a NULL loss leaves the field as it is
    c.log.copy_(canary_log(c.row_floats))
    c.run(1.0, loss=False)
    again = log_bits(c.log)
    assert again[lo] == CANARY and np.array_equal(again[lo + 1:], first[lo + 1:])


def test_grad_stats_captured(grad_case):
    c = grad_case
    c.set_total(2.0)
    c.row.fill_(0)
    c.run(0.5)  # (eager once: the kernels are loaded before the capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.partial()
        c.stand_in_step()
        c.store(0.5)
    rng = np.random.default_rng(5)
    try:
        for row, total in ((1, 7.5), (3, 0.01)):
            data = c.g * F32(rng.uniform(0.5, 2.0)) + rng.standard_normal(c.g.size).astype(F32) * F32(0.1)
            c.grad.set(data)
            c.set_total(total)
            c.row.fill_(row)
            c.log.copy_(canary_log(c.row_floats))
            g.replay()
            torch.cuda.synchronize()
            replayed = log_bits(c.log)
            c.log.copy_(canary_log(c.row_floats))
            c.run(0.5)
            assert np.array_equal(log_bits(c.log), replayed), row
            c.check_row(row, data, total, 0.5)
    finally:
        c.grad.set(c.g)


# ---------------------------------------------------------------------------------------------------------------- spike counts
def _spike_sources(nsrc, n_words, seed):
    rng = np.random.default_rng(seed)
    host, dev, keep = [], [], []
    for k in range(nsrc):
        w = rng.integers(-2 ** 31, 2 ** 31, size=n_words, dtype=np.int64).astype(np.int32)
        w[rng.integers(0, n_words)] = [0, -1, -2 ** 31][k % 3]
        if k % 5 == 4:
            w[:] = 0
        buf = torch.zeros(n_words + 8, dtype=torch.int32, device=DEV)
        shift = k % 4 if nsrc > 1 else 1  # (every 4-byte alignment; a single source sits 4 bytes behind a 16-byte boundary)
        view = buf[shift:shift + n_words]
        view.copy_(torch.from_numpy(w))
        assert view.data_ptr() % 16 == 4 * shift
        host.append(w), dev.append(view), keep.append(buf)
    return host, dev, keep


def _count(dev, n_words, ws, slot0, ws_slots):
    _lib.call("evf_spike_count", (ctypes.c_void_p * 32)(*[t.data_ptr() for t in dev]), len(dev), n_words, _lib.ptr(ws), slot0, ws_slots)


# (5, 33975): 32 parts of 256 threads stride over 8192 groups of 16 bytes a trip; 33975 words are at least 8492 groups at each
# of the four alignments of the five sources, so block 0 takes a second trip and the tail exists
@pytest.mark.parametrize("nsrc,n_words", [(nsrc, n) for nsrc in (1, 5, 32) for n in (1, 63, 64, 1000, 2 * 32 * 32)] + [(5, 33975)])
def test_spike_counts_and_rates(nsrc, n_words):
    parts = int(_lib.load().evf_spike_count_parts())
    host, dev, _keep = _spike_sources(nsrc, n_words, seed=nsrc * 10007 + n_words)
    slot0, ws_slots = 3, nsrc + 5
    ws = torch.full((ws_slots, parts), -7, dtype=torch.int32, device=DEV)
    _count(dev, n_words, ws, slot0, ws_slots)
    got = ws.cpu().numpy().astype(np.int64)
    counts = [ref.bit_count(w) for w in host]
    assert (got[:slot0] == -7).all() and (got[slot0 + nsrc:] == -7).all()
    assert [int(r.sum()) for r in got[slot0:slot0 + nsrc]] == counts
    # rates: slot s belongs to layer (s - slot0) % nlayers; the slots in front of slot0 are given zero partials
    ws[:slot0] = 0
    nlayers = min(nsrc, 7)
    total = -(-nsrc // nlayers) * n_words * 32
    layer = [0] * slot0 + [k % nlayers for k in range(nsrc)]
    row_floats = OFFSET + nlayers + SPARE
    log = canary_log(row_floats)
    row = torch.tensor([1], dtype=torch.int64, device=DEV)
    _lib.call("evf_spike_rates_store", _lib.ptr(ws), ws_slots, (ctypes.c_int * 256)(*layer), len(layer), nlayers, total, _lib.ptr(row),
              NROWS, _lib.ptr(log), row_floats, OFFSET)
    out = log.cpu().numpy()
    lo = row_floats + OFFSET
    for l in range(nlayers):
        want = ref.rate(sum(c for k, c in enumerate(counts) if k % nlayers == l), total)
        assert ref.bits(out[lo + l]) == ref.bits(want), (l, out[lo + l], want)
    inside = np.zeros(out.size, bool)
    inside[lo:lo + nlayers] = True
    assert (log_bits(log)[~inside] == CANARY).all()


def test_spike_log_discipline_and_capture():
    n_words, nsrc, nlayers = 1000, 5, 2
    parts = int(_lib.load().evf_spike_count_parts())
    host, dev, _keep = _spike_sources(nsrc, n_words, seed=3)
    ws = torch.zeros((nsrc, parts), dtype=torch.int32, device=DEV)
    layer = (ctypes.c_int * 256)(*[k % nlayers for k in range(nsrc)])
    total = 3 * n_words * 32
    row_floats = OFFSET + nlayers + SPARE
    log = canary_log(row_floats)
    row = torch.zeros(1, dtype=torch.int64, device=DEV)

    def both():
        _count(dev, n_words, ws, 0, nsrc)
        _lib.call("evf_spike_rates_store", _lib.ptr(ws), nsrc, layer, nsrc, nlayers, total, _lib.ptr(row), NROWS, _lib.ptr(log),
                  row_floats, OFFSET)

    for word in (-1, NROWS):
        row.fill_(word)
        both()
        assert (log_bits(log) == CANARY).all(), word
    row.fill_(2)
    both()
    first = log_bits(log)
    lo = 2 * row_floats + OFFSET
    inside = np.zeros(first.size, bool)
    inside[lo:lo + nlayers] = True
    assert (first[~inside] == CANARY).all() and (first[inside] != CANARY).all()
    both()
    assert np.array_equal(log_bits(log), first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    rng = np.random.default_rng(8)
    for r in (0, 3):
        for k, t in enumerate(dev):
            host[k] = rng.integers(-2 ** 31, 2 ** 31, size=n_words, dtype=np.int64).astype(np.int32)
            t.copy_(torch.from_numpy(host[k]))
        row.fill_(r)
        log.copy_(canary_log(row_floats))
        g.replay()
        torch.cuda.synchronize()
        replayed = log_bits(log)
        log.copy_(canary_log(row_floats))
        both()
        assert np.array_equal(log_bits(log), replayed)
        out = log.cpu().numpy()
        for l in range(nlayers):
            want = ref.rate(sum(ref.bit_count(w) for k, w in enumerate(host) if k % nlayers == l), total)
            assert ref.bits(out[r * row_floats + OFFSET + l]) == ref.bits(want)


# ---------------------------------------------------------------------------------------------------------------- guards
def test_guards_answer_einval_and_write_nothing(grad_case):
    c = grad_case
    lib = _lib.load()
    parts = int(lib.evf_spike_count_parts())
    c.log.copy_(canary_log(c.row_floats))
    c.ws.set(np.full(c.ws_floats, 3.0, F32))
    c.row.fill_(0)
    sws = torch.full((8, parts), -7, dtype=torch.int32, device=DEV)
    words = torch.zeros(64 + 8, dtype=torch.int32, device=DEV)
    srcs = lambda *p: (ctypes.c_void_p * 32)(*p)  # noqa: E731
    five = [words.data_ptr()] * 5
    layer = (ctypes.c_int * 256)(*[k % 2 for k in range(5)])

    ok_p = [c.grad.ptr, _lib.ptr(c.seg_off), _lib.ptr(c.seg_n), c.nseg, c.max_n, c.ws.ptr, c.ws_floats]
    ok_s = [c.ws.ptr, c.ws_floats, _lib.ptr(c.seg_n), c.nseg, c.max_n, _lib.ptr(c.norm_ws), 1.0, _lib.ptr(c.loss), _lib.ptr(c.row),
            NROWS, _lib.ptr(c.log), c.row_floats, OFFSET]
    ok_c = [srcs(*five), 5, 64, _lib.ptr(sws), 2, 8]
    ok_r = [_lib.ptr(sws), 8, layer, 5, 2, 5 * 64 * 32, _lib.ptr(c.row), NROWS, _lib.ptr(c.log), c.row_floats, OFFSET]

    def bad(name, ok, **change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        assert rc_of(name, *args) == EINVAL, (name, change)

    for i in (0, 1, 2, 5):
        bad("evf_grad_stats_partial", ok_p, **{f"a{i}": None})
    for v in (0, -1):
        bad("evf_grad_stats_partial", ok_p, a3=v)
        bad("evf_grad_stats_partial", ok_p, a4=v)
    bad("evf_grad_stats_partial", ok_p, a6=c.ws_floats - 1)
    bad("evf_grad_stats_partial", ok_p, a0=c.grad.ptr + 2)
    bad("evf_grad_stats_partial", ok_p, a5=c.ws.ptr + 1)
    bad("evf_grad_stats_partial", ok_p, a1=_lib.ptr(c.seg_off) + 4)
    bad("evf_grad_stats_partial", ok_p, a2=_lib.ptr(c.seg_n) + 4)

    for i in (0, 2, 5, 8, 10):
        bad("evf_grad_stats_store", ok_s, **{f"a{i}": None})
    for v in (0, -1):
        for i in (3, 4, 9, 11):
            bad("evf_grad_stats_store", ok_s, **{f"a{i}": v})
    bad("evf_grad_stats_store", ok_s, a12=-1)
    bad("evf_grad_stats_store", ok_s, a12=OFFSET + SPARE + 1)
    bad("evf_grad_stats_store", ok_s, a1=c.ws_floats - 1)
    bad("evf_grad_stats_store", ok_s, a0=c.ws.ptr + 2)
    bad("evf_grad_stats_store", ok_s, a10=_lib.ptr(c.log) + 2)
    bad("evf_grad_stats_store", ok_s, a2=_lib.ptr(c.seg_n) + 4)
    bad("evf_grad_stats_store", ok_s, a8=_lib.ptr(c.row) + 4)

    bad("evf_spike_count", ok_c, a0=None)
    bad("evf_spike_count", ok_c, a3=None)
    for v in (0, -1, 33):
        bad("evf_spike_count", ok_c, a1=v, a5=64)
    for v in (0, -1, 2 ** 31):
        bad("evf_spike_count", ok_c, a2=v)
    bad("evf_spike_count", ok_c, a4=-1)
    bad("evf_spike_count", ok_c, a4=4)  # a short ws: slots 4 .. 8 of 8
    bad("evf_spike_count", ok_c, a3=_lib.ptr(sws) + 2)
    bad("evf_spike_count", ok_c, a0=srcs(*(five[:3] + [None] + five[4:])))
    bad("evf_spike_count", ok_c, a0=srcs(*(five[:4] + [words.data_ptr() + 2])))

    for i in (0, 2, 6, 8):
        bad("evf_spike_rates_store", ok_r, **{f"a{i}": None})
    for v in (0, -1, 257):
        bad("evf_spike_rates_store", ok_r, a3=v, a1=1024)
        bad("evf_spike_rates_store", ok_r, a4=v)
    for v in (0, -1):
        for i in (5, 7, 9):
            bad("evf_spike_rates_store", ok_r, **{f"a{i}": v})
    bad("evf_spike_rates_store", ok_r, a1=4)  # a short ws
    bad("evf_spike_rates_store", ok_r, a2=(ctypes.c_int * 256)(0, 1, 2, 0, 1))
    bad("evf_spike_rates_store", ok_r, a10=-1)
    bad("evf_spike_rates_store", ok_r, a10=c.row_floats - 1)
    bad("evf_spike_rates_store", ok_r, a0=_lib.ptr(sws) + 2)
    bad("evf_spike_rates_store", ok_r, a8=_lib.ptr(c.log) + 2)
    bad("evf_spike_rates_store", ok_r, a6=_lib.ptr(c.row) + 4)

    torch.cuda.synchronize()
    assert (log_bits(c.log) == CANARY).all()
    assert (c.ws.get() == 3.0).all() and bool((sws == -7).all())
    c.bufs.check()
    # ... and the accepted forms of the same arguments
    for name, ok in (("evf_grad_stats_partial", ok_p), ("evf_grad_stats_store", ok_s), ("evf_spike_count", ok_c),
                     ("evf_spike_rates_store", ok_r)):
        assert rc_of(name, *ok) == 0, name
    torch.cuda.synchronize()
