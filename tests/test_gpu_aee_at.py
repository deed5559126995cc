"""evf_aee_at (csrc/evf_eval_log.hip) through the C ABI on the MI355X against the float64 reference of tests/aee_at_ref.py: the
valid and the outlier counts exactly, the error sum at the derived bound (d + 8) 2^-24 -- against float64 and against the
existing evf_aee --, the row formed from the sums bit for bit, rows outside the log, inf / nan of a sample with dt_input = 0,
two calls bit for bit, a captured call replayed under another row word, and every host guard."""

import numpy as np
import pytest
import torch

import aee_at_ref as R
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32, F64 = np.float32, np.float64
#          scalar   vector, one stripe   one stripe, 16-byte loads, exactly full   three stripes, a short last one (scalar / vector)
SHAPES = [(15, 21), (16, 24), (32, 64), (45, 91), (48, 92)]
NROWS, ROW_FLOATS, OFFSET = 4, 19, 5


class Case:
    """The device side of one set of inputs: every float32 operand between guards, the doubles, a log full of NaN canaries."""

    def __init__(self, i, shift=0):
        self.i, self.bufs = i, Bufs()
        self.B, _, self.H, self.W = i["flow"].shape
        self.S = R.stripes(self.H, self.W)
        self.flow, self.gt, self.mask = (self.bufs.new(i[k], shift) for k in ("flow", "gt", "mask"))
        self.ws = self.bufs.new(np.full(self.B * self.S * 3, 7.0, F32))
        self.dt_gt, self.dt_input = (torch.from_numpy(np.array(i[k], F64)).to(DEV) for k in ("dt_gt", "dt_input"))
        self.row = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.log = torch.full((NROWS, ROW_FLOATS), float("nan"), dtype=torch.float32, device=DEV)

    def args(self):
        return [self.flow.ptr, self.gt.ptr, self.mask.ptr, self.dt_gt.data_ptr(), self.dt_input.data_ptr(), self.B, self.H, self.W,
                R.FLOW_SCALING, self.row.data_ptr(), NROWS, self.log.data_ptr(), ROW_FLOATS, OFFSET, self.ws.ptr, self.B * self.S * 3]

    def call(self, row):
        self.row.fill_(row)
        return _lib.raw("evf_aee_at", *self.args())

    def stored(self):
        """-> (row index, the 2 (B + 1) floats) of the one row that holds anything; everything else must still be NaN."""
        log = self.log.cpu().numpy()
        rows = [r for r in range(NROWS) if not np.isnan(log[r, OFFSET])]
        assert len(rows) == 1, log
        n = 2 * (self.B + 1)
        rest = log.copy()
        rest[rows[0], OFFSET:OFFSET + n] = np.nan
        assert np.isnan(rest).all(), "a store outside the row's 2 (B + 1) floats"
        return rows[0], log[rows[0], OFFSET:OFFSET + n].copy()

    def sums(self):
        return self.ws.get().reshape(self.B, self.S, 3)[:, 0].astype(F64)


def test_stripes_follow_the_geometry():
    lib = _lib.load()
    for H, W in SHAPES + [(256, 256), (1, 1), (1, 2048), (1, 2049)]:
        assert lib.evf_aee_at_stripes(H, W) == R.stripes(H, W)
    assert [R.stripes(*s) for s in SHAPES] == [1, 1, 1, 2, 3] and 45 * 91 % R.STRIPE and 48 * 92 % R.STRIPE
    assert lib.evf_aee_at_stripes(0, 4) == EINVAL and lib.evf_aee_at_stripes(4, -1) == EINVAL
    assert lib.evf_aee_at_stripes(65536, 32768) == EINVAL


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_counts_exact_sum_at_the_bound_rows_in_place(H, W, B):
    i = R.make(B, H, W)
    se64, nv64, no64, margin = R.sums(i)
    assert margin >= 1e-3  # every comparison clears its threshold: the counts are decided
    flat = lambda a: np.asarray(a).reshape(B, -1)  # noqa: E731
    assert (flat(i["mask"]) == 0).any() and ((flat(i["gt"][:, 0]) == 0) & (flat(i["gt"][:, 1]) == 0)).any()
    assert (0 < no64).all() and (no64 < nv64).all() and (nv64 < H * W).all()  # (errors on both sides of the thresholds)
    c = Case(i)
    for bad in (-1, NROWS, NROWS + 5, -(2 ** 40)):  # a row outside the log stores nothing
        assert c.call(bad) == 0
    torch.cuda.synchronize()
    assert torch.isnan(c.log).all()
    assert c.call(2) == 0
    at, got = c.stored()
    assert at == 2
    sums = c.sums()
    print((B, H, W), "d", R.chain(H, W), "sum err rel. error", np.abs(sums[:, 0] - se64) / se64, "bound", R.bound(H, W))
    assert np.array_equal(sums[:, 1], nv64) and np.array_equal(sums[:, 2], no64)  # counts: exactly
    assert (np.abs(sums[:, 0] - se64) <= R.bound(H, W) * se64).all()
    assert np.array_equal(got.view(np.uint32), R.row(*sums.T).view(np.uint32))  # the row: launch 2's float32 operations on the sums
    # percent_b is AEE.forward's: the same float32 operations on the same (exact) counts
    out = torch.from_numpy(np.stack([se64, nv64, no64], 1).astype(F32))
    assert np.array_equal(got[B + 1:2 * B + 1], (out[:, 2].sum() / (out[:, 1] + 1e-9)).numpy())
    # the existing one-block kernel on the same inputs (the ratio handed over as float32)
    old = torch.full((B, 3), -1.0, dtype=torch.float32, device=DEV)
    ratio = torch.from_numpy(R.ratio32(i["dt_gt"], i["dt_input"])).to(DEV)
    assert _lib.raw("evf_aee", c.flow.ptr, c.gt.ptr, c.mask.ptr, ratio.data_ptr(), B, H, W, R.FLOW_SCALING, old.data_ptr()) == 0
    old = old.cpu().numpy().astype(F64)
    assert np.array_equal(old[:, 1:], sums[:, 1:])
    assert (np.abs(sums[:, 0] - old[:, 0]) <= R.bound(H, W) * old[:, 0]).all()
    # a second call: bit for bit, in another row
    assert c.call(0) == 0
    log = c.log.cpu().numpy()
    assert np.array_equal(log[0, OFFSET:OFFSET + 2 * (B + 1)].view(np.uint32), got.view(np.uint32))
    c.bufs.check()


@pytest.mark.parametrize("H,W", [(16, 24), (48, 92)])
def test_misaligned_operands_take_the_scalar_path(H, W):
    """W % 4 == 0 but the tensors 4 bytes off a 16-byte boundary: dword loads, the same counts, the sum at the same bound."""
    i = R.make(2, H, W)
    se64, nv64, no64, _ = R.sums(i)
    c = Case(i, shift=1)
    assert c.flow.ptr % 16 == 4 and c.call(1) == 0
    _at, _got = c.stored()
    sums = c.sums()
    assert np.array_equal(sums[:, 1], nv64) and np.array_equal(sums[:, 2], no64)
    assert (np.abs(sums[:, 0] - se64) <= R.bound(H, W) * se64).all()
    c.bufs.check()


@pytest.mark.parametrize("broken", ["inf", "nan"])
@pytest.mark.parametrize("B", [2, 3])
def test_a_sample_with_dt_input_zero_is_what_float32_torch_gives(B, broken):
    H, W = 45, 91
    i = R.make(B, H, W, broken)
    se64, nv64, no64, margin = R.sums(i)
    assert margin >= 1e-3
    c = Case(i)
    assert c.call(3) == 0
    _at, got = c.stored()
    sums = c.sums()
    assert np.array_equal(sums[:, 1], nv64) and np.array_equal(sums[:, 2], no64)
    assert (np.abs(sums[:-1, 0] - se64[:-1]) <= R.bound(H, W) * se64[:-1]).all()
    # the float32 torch operations of AEE.forward and the reference's AEE (loss/flow.py:594-628) on the CPU
    T = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    flow, gt, mask = T(i["flow"]), T(i["gt"]), T(i["mask"])
    ratio = torch.as_tensor(T(i["dt_gt"]), dtype=torch.float32) / torch.as_tensor(T(i["dt_input"]), dtype=torch.float32)
    fl = flow * R.FLOW_SCALING * ratio.view(B, 1, 1, 1)
    valid = (mask != 0) & ~((gt[:, 0] == 0) & (gt[:, 1] == 0))
    err = torch.where(valid, (fl - gt).pow(2).sum(1).sqrt(), torch.zeros(()))
    se = err.view(B, -1).sum(1)
    aee = (se / (valid.view(B, -1).sum(1).float() + 1e-9)).numpy()
    assert (np.isinf(aee[-1]) and aee[-1] > 0) if broken == "inf" else np.isnan(aee[-1])
    assert np.array_equal(np.isnan(got[:B]), np.isnan(aee)) and np.array_equal(np.isinf(got[:B]), np.isinf(aee))
    assert got[B - 1].view(np.uint32) == aee[B - 1:].view(np.uint32)[0] or np.isnan(aee[-1])  # +inf bit for bit / a NaN
    assert np.isfinite(got[:B - 1]).all() and (np.isinf(got[B]) if broken == "inf" else np.isnan(got[B]))  # the batch mean follows
    assert np.array_equal(got.view(np.uint32)[B + 1:], R.row(*sums.T).view(np.uint32)[B + 1:]) and np.isfinite(got[B + 1:]).all()
    c.bufs.check()


def test_a_captured_call_follows_the_row_word():
    i = R.make(2, 45, 91)
    c = Case(i)
    assert c.call(1) == 0  # (not captured: the kernels are loaded)
    _at, want = c.stored()
    c.log.fill_(float("nan"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        assert _lib.raw("evf_aee_at", *c.args()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(c.log).all()  # captured, not run
    for r in (3, -1, 0):
        c.log.fill_(float("nan"))
        c.row.fill_(r)
        g.replay()
        torch.cuda.synchronize()
        if r < 0:
            assert torch.isnan(c.log).all()
        else:
            at, got = c.stored()
            assert at == r and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    c.bufs.check()


def test_host_guards():
    i = R.make(2, 16, 24)
    c = Case(i)
    ok = c.args()
    assert _lib.raw("evf_aee_at", *ok) == 0
    _at, _got = c.stored()
    c.log.fill_(float("nan"))
    bad = [(k, None) for k in (0, 1, 2, 3, 4, 9, 11, 14)]                       # null pointers
    bad += [(k, v) for k in (5, 6, 7, 10, 12) for v in (0, -1)]                  # non-positive B, H, W, nrows, row_floats
    bad += [(5, 65536), (13, -1), (13, ROW_FLOATS - 2 * 3 + 1), (12, OFFSET + 2 * 3 - 1)]  # B, offset + 2 (B + 1) > row_floats
    bad += [(15, 2 * 1 * 3 - 1), (15, 0), (15, -4)]                              # a workspace smaller than B S 3 floats
    bad += [(11, ok[11] + 2), (14, ok[14] + 1), (0, ok[0] + 2), (3, ok[3] + 4), (9, ok[9] + 4)]  # misaligned log, ws, flow, dt_gt, row
    for at, value in bad:
        args = list(ok)
        args[at] = value
        assert _lib.raw("evf_aee_at", *args) == EINVAL, (at, value)
    assert _lib.raw("evf_aee_at", *[ok[k] if k != 13 else ROW_FLOATS - 2 * 3 for k in range(16)]) == 0  # the last offset that fits
    torch.cuda.synchronize()
    log = c.log.cpu().numpy()
    assert np.isnan(log[:, :ROW_FLOATS - 6]).all() and not np.isnan(log[0, ROW_FLOATS - 6:]).any()  # no refused call stored anything
    c.bufs.check()
