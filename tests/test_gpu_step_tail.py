"""The tail of a training step through the C ABI against plain references (tests/step_tail_ref.py):
clip + Adam (evf_clip_adam_step, evf_clip_adam_fused, train.FlatAdam) against the fp64 reference, teacher-forced over 12 steps,
within the bounds that tests/test_host_step_tail_reference.py establishes on the CPU; the gradient collection
(evf_grads_finalize, evf_reduce_slabs, evf_reduce_slabs_multi, evf_sum_rows, evf_add_segments, evf_unpack_conv_wgrad) on
integer-valued inputs, where every sum is exact in fp32 in any order, BIT FOR BIT against the int64 / fp64 reference, plus one
real-valued case per kernel.  Every buffer handed to a kernel sits between 64 guard elements on either side."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import step_tail_ref as R
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32 = np.float32


def call(name, *args):
    """Status of an entry point on torch's current stream."""
    return _lib.raw(name, *args)


def ptrs(bufs):
    return (ctypes.c_void_p * max(len(bufs), 1))(*[b.ptr for b in bufs])


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def assert_bits(got, ref64, what):
    """got (fp32 from the device) == the exact reference, bit for bit."""
    ref = np.asarray(ref64, np.float64)
    assert np.array_equal(ref, ref.astype(F32).astype(np.float64)), "the reference is not exact in fp32"
    ref32 = ref.astype(F32)
    got = np.asarray(got, F32).reshape(ref32.shape)
    bad = np.flatnonzero((got.view(np.int32) != ref32.view(np.int32)).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[0]}: {got.reshape(-1)[bad[0]]} != {ref32.reshape(-1)[bad[0]]}"


def assert_close_sum(got, ref64, abs_sum, what):
    """Real-valued sums: |got - ref| <= 64 * 2^-24 * sum |x| per output (the longest addition chain of the kernels, at most 64
    terms, times the unit round-off)."""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(ref64).reshape(-1))
    bound = 64.0 * R.U * np.asarray(abs_sum, np.float64).reshape(-1)
    i = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: error {err[i]:.3g} > bound {bound[i]:.3g} at {i}"


# ================================================================================================================= Adam
ADAM = ("evf_clip_adam_step", "evf_clip_adam_fused")
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 16 * 1024 - 1, 16 * 1024, 16 * 1024 + 3, 75011, 2 ** 20, 2 ** 20 + 1)


def run_adam(entry, n, rg, device_step, zero_grad, shift=0):
    """12 teacher-forced steps of one entry point; asserts the bounds, the workspace, the gradient buffer and the guards."""
    p0, max_norm, gs = R.case_inputs(n, rg)
    B = Bufs()
    zeros = np.zeros(n, F32)
    bp, bm, bv, bg, ws = B.new(p0), B.new(zeros), B.new(zeros), B.new(zeros, shift=shift), B.new(np.zeros(8, F32))
    p, m, v = p0, zeros, zeros
    worst = dict.fromkeys(("p", "m", "v"), 0.0)
    for t, g in enumerate(gs, 1):
        bg.set(g)
        rc = call(entry, bp.ptr, bg.ptr, bm.ptr, bv.ptr, n, max_norm, R.LR, R.B1, R.B2, R.EPS, 0 if device_step else t, ws.ptr,
                  zero_grad)
        assert rc == 0, (entry, rc)
        got = (bp.get(), bm.get(), bv.get())
        w = ws.get()
        e = R.normalised_errors(got + (w[0],), (p, m, v), g, max_norm=max_norm, t=t)
        for k in worst:
            worst[k] = max(worst[k], e[k])
            assert e[k] <= R.BOUND[k], f"{entry} n={n} {rg} step {t}: {k} error {e[k]:.3g} units > {R.BOUND[k]:.3g} ({e})"
        assert w[1] == (t if device_step else 0), f"step counter {w[1]} after step {t}"
        assert not w.view(np.int32)[2:].any(), f"workspace words 2.. after step {t}: {w}"
        ga = bg.get()
        if zero_grad:
            assert not ga.view(np.int32).any(), "zero_grad = 1 left something in the gradient buffer"
        else:
            assert same_bits(ga, g), "zero_grad = 0 changed the gradient buffer"
        p, m, v = got
    B.check()
    return worst


@pytest.mark.parametrize("entry", ADAM)  # (varies fastest: both entry points run on the inputs of a size before the next)
@pytest.mark.parametrize("rg", R.REGIMES)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_against_fp64(entry, n, rg):
    """Sizes: the n % 4 tail; the one / two block boundary; the slice partition of the fused kernel around 16 x 1024; a FireNet's
    parameter count; the largest fused size and the first one that falls through to the two launches.  Step counter from the
    host and on the device, zero_grad on and off (all four combinations up to 16 k elements, two of them above)."""
    combos = [(0, 1), (1, 0), (0, 0), (1, 1)] if n <= 16 * 1024 + 3 else [(0, 1), (1, 0)]
    for device_step, zero_grad in combos:
        worst = run_adam(entry, n, rg, device_step, zero_grad)
    print(f"{entry} n={n} {rg}: " + "  ".join(f"{k} {x:.3g}" for k, x in worst.items()))


@pytest.mark.parametrize("n", (5, 1025, 75011))
@pytest.mark.parametrize("entry", ADAM)
def test_adam_with_a_gradient_that_is_not_16_byte_aligned(entry, n):
    """The fused entry point's fall-through to the two launches, and the scalar branch of k_sumsq."""
    for rg, device_step, zero_grad in (("clipped", 1, 1), ("none", 0, 0)):
        run_adam(entry, n, rg, device_step, zero_grad, shift=1)


@pytest.mark.parametrize("entry", ADAM)
def test_adam_norm_of_integer_gradients_is_exact(entry):
    """Integer-valued gradients in [-3, 3] at n = 2^20: the sum of squares is exact in fp32 in any order."""
    n = 2 ** 20
    g = np.random.default_rng(5).integers(-3, 4, n).astype(F32)
    exact = int(np.sum(g.astype(np.int64) ** 2))
    assert exact < 2 ** 24
    B = Bufs()
    zeros = np.zeros(n, F32)
    bp, bm, bv, bg, ws = B.new(zeros), B.new(zeros), B.new(zeros), B.new(g), B.new(np.zeros(8, F32))
    for step in (1, 0):  # host counter, device counter
        bg.set(g)
        assert call(entry, bp.ptr, bg.ptr, bm.ptr, bv.ptr, n, 100.0, R.LR, R.B1, R.B2, R.EPS, step, ws.ptr, 1) == 0
        w = ws.get()
        assert w[0] == float(exact) and float(w[0]).is_integer(), (w[0], exact)
    B.check()


@pytest.mark.parametrize("entry", ADAM)
def test_adam_bad_arguments_change_nothing(entry):
    n = 1025
    p0, max_norm, gs = R.case_inputs(n, "clipped")
    B = Bufs()
    data = [p0, gs[0], gs[1], np.abs(gs[2]), np.array([0, 3, 0, 0, 0, 0, 0, 0], F32)]
    b = [B.new(d) for d in data]
    for missing in range(5):
        a = [None if i == missing else x.ptr for i, x in enumerate(b)]
        assert call(entry, a[0], a[1], a[2], a[3], n, 1e-4, R.LR, R.B1, R.B2, R.EPS, 0, a[4], 1) == EINVAL
    for bad_n in (0, -4):
        assert call(entry, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, bad_n, 1e-4, R.LR, R.B1, R.B2, R.EPS, 0, b[4].ptr, 1) == EINVAL
    for x, d in zip(b, data):
        assert same_bits(x.get(), d)
    B.check()


# ------------------------------------------------------------------------------------------------------------ FlatAdam
def _torch_adam_fp64(p, g, m, v, t, max_norm):
    """One step of clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU from the given state -> p', m', v', |g|^2."""
    f = lambda x: float(F32(x))  # noqa: E731  (the hyper-parameters as the C ABI sees them)
    w = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([w], lr=f(R.LR), betas=(f(R.B1), f(R.B2)), eps=f(R.EPS))
    opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                    "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    w.grad = torch.from_numpy(g.astype(np.float64))
    sumsq = float(w.grad.square().sum())
    if max_norm:
        torch.nn.utils.clip_grad_norm_([w], f(max_norm))
    opt.step()
    return w.detach().numpy(), opt.state[w]["exp_avg"].numpy(), opt.state[w]["exp_avg_sq"].numpy(), sumsq


@pytest.mark.parametrize("clip", (None, "active"))
@pytest.mark.parametrize("device_step", (False, True))
@pytest.mark.parametrize("fused", (True, False))
def test_flat_adam_against_torch_adam_fp64(monkeypatch, fused, device_step, clip):
    from event_flow_amd import train
    from event_flow_amd.models import hip_ops

    monkeypatch.setattr(train, "FUSED_ADAM", fused)
    monkeypatch.setattr(hip_ops, "DIRECT_PARAM_GRADS", hip_ops.DIRECT_PARAM_GRADS)  # (FlatAdam switches it on: restored)
    shapes = [(7,), (33, 5), (1,)]
    n = sum(int(np.prod(s)) for s in shapes)
    p0, max_norm, gs = R.case_inputs(n, "clipped" if clip else "none")

    class Three(torch.nn.Module):
        def __init__(self):
            super().__init__()
            off = 0
            for name, s in zip("abc", shapes):
                k = int(np.prod(s))
                setattr(self, name, torch.nn.Parameter(torch.from_numpy(p0[off:off + k].reshape(s).copy())))
                off += k

    model = Three().to(DEV)
    opt = train.FlatAdam(model, lr=R.LR, betas=(R.B1, R.B2), eps=R.EPS, clip=max_norm if clip else None, device_step=device_step)
    try:
        params = [model.a, model.b, model.c]
        p, m, v = p0, np.zeros(n, F32), np.zeros(n, F32)
        for t, g in enumerate(gs, 1):
            off = 0
            for q in params:
                q.grad.copy_(torch.from_numpy(g[off:off + q.numel()].reshape(q.shape).copy()))
                off += q.numel()
            opt.mark_grad_dirty()
            opt.step()
            got = (np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in params]), opt.m.cpu().numpy(), opt.v.cpu().numpy())
            ref = _torch_adam_fp64(p, g, m, v, t, max_norm)
            e = R.normalised_errors(got + (float(opt.norm_ws[0]),), (p, m, v), g, max_norm=max_norm, t=t, ref=ref)
            for k in ("p", "m", "v"):
                assert e[k] <= R.BOUND[k], f"step {t}: {k} error {e[k]:.3g} units > {R.BOUND[k]:.3g} ({e})"
            norm = np.sqrt(ref[3])
            assert abs(opt.grad_norm() - norm) <= R.BOUND["sumsq"] * norm, (t, opt.grad_norm(), norm)
            for q in params:
                assert q.grad is not None and not bool(q.grad.any()), "`.grad` must read zeros after step()"
            assert same_bits(got[0], opt.flat_param.cpu().numpy())  # the parameters ARE views of the flat buffer
            p, m, v = got
        assert opt.steps == 12 and float(opt.norm_ws[1]) == (12.0 if device_step else 0.0)
    finally:
        opt.close()


# ================================================================================================== gradient collection
NW = R.NW
NSLABS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
_MULT = (1, 5, 7, 11, 13, 17, 19, 23, 25, 29, 31, 35, 37, 41, 43, 47)  # coprime to 9216: e -> e * k mod 9216 is a bijection


@functools.lru_cache(maxsize=None)
def _noise():
    a = np.random.default_rng(11).integers(-8, 9, (300, NW)).astype(F32)
    a.setflags(write=False)
    return a


def slab_input(t, nslab, real=False):
    """[nslab][9*32*32] partial sums of weight tensor t.  Slab 0 holds a DIFFERENT integer for every (tap, ci, co) (a permutation
    of -4608 .. 4607 that depends on t), so that no wrong transposition can pass; the other slabs integers in [-8, 8].  Every
    partial sum stays far below 2^24: exact in fp32 in any order.  real: the same times a real factor per element."""
    x = np.roll(_noise()[:nslab], 97 * t, axis=1).copy()
    x[0] = (np.arange(NW) * _MULT[t]) % NW - NW // 2
    if real:
        x = x * np.random.default_rng(100 + t).uniform(0.5, 1.5, x.shape).astype(F32)
    return x.astype(F32)


def ints_like(shape, seed, real=False):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, shape).astype(F32)
    return (x * rng.uniform(0.5, 1.5, shape)).astype(F32) if real else x


def _check_slab_result(got, slabs, dst0, real, what):
    ref = R.reduce_slabs_ref(slabs, dst0)
    if real:
        abs_sum = R.reduce_slabs_ref(np.abs(slabs), np.abs(dst0) if dst0 is not None else None)
        assert_close_sum(got, ref, abs_sum, what)
    else:
        assert_bits(got, ref, what)


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("nslab", NSLABS + ("real",))
def test_reduce_slabs(nslab, accumulate):
    real = nslab == "real"
    nslab = 300 if real else nslab
    B = Bufs()
    slabs, dst0 = slab_input(3, nslab, real), ints_like((32, 32, 3, 3), 40, real)
    bs, bd = B.new(slabs), B.new(dst0)
    assert call("evf_reduce_slabs", bs.ptr, nslab, NW, accumulate, bd.ptr) == 0
    _check_slab_result(bd.get(), slabs, dst0 if accumulate else None, real, f"evf_reduce_slabs nslab={nslab}")
    assert same_bits(bs.get(), slabs)
    B.check()


@pytest.mark.parametrize("nslab", NSLABS + ("real",))
@pytest.mark.parametrize("count", (1, 3, 16))
def test_multi_tensor_slab_reductions(count, nslab):
    """evf_reduce_slabs_multi and the slab part of evf_grads_finalize (no segments: nseg = 0) on the same inputs."""
    real = nslab == "real"
    nslab = 257 if real else nslab
    B = Bufs()
    slabs = [slab_input(t, nslab, real) for t in range(count)]
    dst0 = [ints_like((32, 32, 3, 3), 50 + t, real) for t in range(count)]
    bs = [B.new(s) for s in slabs]
    bd_multi, bd_fin = [B.new(d) for d in dst0], [B.new(d) for d in dst0]
    assert call("evf_reduce_slabs_multi", ptrs(bs), ptrs(bd_multi), count, nslab, NW) == 0
    assert call("evf_grads_finalize", ptrs(bs), ptrs(bd_fin), count, nslab, None, 1, None, 0, 0, None, 0, 0, 0,
                None, None, None, None, 0) == 0
    for t in range(count):
        _check_slab_result(bd_multi[t].get(), slabs[t], dst0[t], real, f"evf_reduce_slabs_multi tensor {t}/{count} nslab={nslab}")
        _check_slab_result(bd_fin[t].get(), slabs[t], dst0[t], real, f"evf_grads_finalize tensor {t}/{count} nslab={nslab}")
        assert same_bits(bs[t].get(), slabs[t])
    B.check()


def test_slab_reductions_status_paths():
    """0 or 17 tensors and n != 9216: the documented status, nothing written."""
    B = Bufs()
    slabs, dst0 = slab_input(0, 2), ints_like((32, 32, 3, 3), 60)
    bs, bd = B.new(slabs), B.new(dst0)
    s17, d17 = ptrs([bs] * 17), ptrs([bd] * 17)
    assert call("evf_reduce_slabs_multi", s17, d17, 0, 2, NW) == EINVAL
    assert call("evf_reduce_slabs_multi", s17, d17, 17, 2, NW) == EINVAL
    assert call("evf_reduce_slabs_multi", s17, d17, 1, 2, NW - 32) == EINVAL
    assert call("evf_reduce_slabs", bs.ptr, 2, NW - 32, 1, bd.ptr) == EINVAL
    assert call("evf_reduce_slabs", bs.ptr, 0, NW, 1, bd.ptr) == EINVAL
    fin = lambda nslabs, nseg: call("evf_grads_finalize", s17, d17, nslabs, 2, None, 1, None, 0, 0, None, 0, 0, 0,  # noqa: E731
                                    None, None, None, None, nseg)
    assert fin(17, 0) == EINVAL
    assert fin(0, 0) == 0  # nothing to do
    assert same_bits(bd.get(), dst0) and same_bits(bs.get(), slabs)
    B.check()


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("real", (False, True))
def test_unpack_conv_wgrad_transposes_tap_ci_co(accumulate, real):
    """[tap][ci][co] -> [co][ci][3][3] on a packed gradient in which every element is a different integer."""
    B = Bufs()
    packed, dst0 = slab_input(5, 1, real), ints_like((32, 32, 3, 3), 70, real)
    assert np.unique(slab_input(5, 1)).size == NW
    bs, bd = B.new(packed), B.new(dst0)
    assert call("evf_unpack_conv_wgrad", bs.ptr, 32, 32, accumulate, bd.ptr) == 0
    _check_slab_result(bd.get(), packed, dst0 if accumulate else None, real, "evf_unpack_conv_wgrad")
    # ... and spelled out, independent of the helper: dst[co][ci][dy][dx] = packed[(dy*3 + dx)][ci][co]
    got, pk = bd.get(), packed.reshape(3, 3, 32, 32)
    if not accumulate and not real:
        for co, ci, dy, dx in ((0, 0, 0, 0), (31, 0, 2, 2), (7, 3, 1, 1), (1, 30, 0, 2), (30, 1, 2, 0)):
            assert got[co, ci, dy, dx] == pk[dy, dx, ci, co]
    assert call("evf_unpack_conv_wgrad", bs.ptr, 32, 16, accumulate, bd.ptr) == EINVAL
    B.check()


@pytest.mark.parametrize("nrows", (1, 15, 16, 17, 127, 128, 129, 700, "real"))
def test_sum_rows(nrows):
    """Both kernels behind evf_sum_rows (nrows >= 128 with accumulate bit 0 takes the second one), all four `accumulate` values:
    bit 0 adds to dst, bit 1 zeroes the rows and touches nothing else."""
    real = nrows == "real"
    for nr in ((127, 700) if real else (nrows,)):
        for n in (1, 16, 17, 64, 65, 160):
            rows0, dst0 = ints_like((nr, n), 80 + n, real), ints_like((n,), 81 + n, real)
            for accumulate in range(4):
                B = Bufs()
                br, bd = B.new(rows0), B.new(dst0)
                assert call("evf_sum_rows", br.ptr, nr, n, accumulate, bd.ptr) == 0
                dref, rref = R.sum_rows_ref(rows0, dst0, accumulate)
                what = f"evf_sum_rows nrows={nr} n={n} accumulate={accumulate}"
                if real:
                    assert_close_sum(bd.get(), dref, np.abs(rows0).sum(axis=0) + (np.abs(dst0) if accumulate & 1 else 0), what)
                else:
                    assert_bits(bd.get(), dref, what)
                rows_after = br.get()
                assert same_bits(rows_after, rref.astype(F32)), what + ": rows"
                B.check()


ADD_LENGTHS = (1, 2, 255, 256, 257, 2049, 75011)


@pytest.mark.parametrize("clear", (0, 1))
@pytest.mark.parametrize("nseg", (1, 5, 32, "real"))
def test_add_segments(nseg, clear):
    real = nseg == "real"
    nseg = 5 if real else nseg
    # (the one-segment case takes the longest length: more elements than the launch has threads)
    lens = [ADD_LENGTHS[-1]] if nseg == 1 else [ADD_LENGTHS[(3 * k + 2) % 7] for k in range(nseg)]
    order = list(range(nseg))[::-1]  # segments need not be sorted by offset
    off, pos = [0] * nseg, 5
    for k in order:
        off[k] = pos
        pos += lens[k] + 7 + k  # a gap behind every segment: elements that belong to none
    src0 = ints_like((pos + 9,), 90, real)
    dst0 = [ints_like((lens[k],), 91 + k, real) for k in range(nseg)]
    B = Bufs()
    bs, bd = B.new(src0), [B.new(d) for d in dst0]
    assert call("evf_add_segments", bs.ptr, ptrs(bd), ints(off), ints(lens), nseg, clear) == 0
    dref, sref = R.add_segments_ref(src0, dst0, off, lens, clear)
    for k in range(nseg):
        if real:
            assert_close_sum(bd[k].get(), dref[k], np.abs(dst0[k]) + np.abs(src0[off[k]:off[k] + lens[k]]), f"segment {k}")
        else:
            assert_bits(bd[k].get(), dref[k], f"evf_add_segments segment {k} of {nseg} (n={lens[k]})")
    assert same_bits(bs.get(), sref.astype(F32)), "source: consumed elements zeroed (clear) / everything else unchanged"
    B.check()
    if not real and not clear:
        assert call("evf_add_segments", bs.ptr, ptrs((bd * 33)[:33]), ints((off * 33)[:33]), ints((lens * 33)[:33]), 33, 0) == EINVAL
        assert call("evf_add_segments", bs.ptr, ptrs(bd), ints(off), ints(lens), 0, 0) == EINVAL
        assert same_bits(bs.get(), sref.astype(F32))


# ---- the segment part of evf_grads_finalize
SEG_N = (2, 32, 63, 64, 65, 576)
SEG_OFF = (3, 11, 50, 130, 200, 300)  # scattered: columns 0-2, 5-10, 43-49, 113-129, 194-199, 265-299, 876.. belong to no segment
HEAD_OFF, NHCOLS, NSMALL = 300, 576, 900
SEG_ORDER = (3, 0, 5, 1, 4, 2)


def _finalize_case(nrows, with_seg_rows, nhrows, ncols, clear_small, real, slab_count=0, nslab=17):
    """One launch of evf_grads_finalize against finalize_ref.  nrows / nhrows None: that source is absent."""
    off, n = [SEG_OFF[k] for k in SEG_ORDER], [SEG_N[k] for k in SEG_ORDER]
    nseg = len(n)
    small0 = ints_like((NSMALL,), 200, real)
    dst0 = [ints_like((k,), 210 + i, real) for i, k in enumerate(n)]
    seg_rows = None
    rows0 = head0 = None
    if nrows is not None:
        rows0 = ints_like((nrows, ncols), 201, real)
        if with_seg_rows:
            # some smaller than nrows, one larger, one 0 (= all rows); rows behind seg_rows[k] hold nothing for segment k
            seg_rows = [max(1, nrows // 2), nrows, 1, nrows + 5, 0, max(1, nrows - 1)]
            for k in range(nseg):
                if 0 < seg_rows[k] < nrows:
                    rows0[seg_rows[k]:, off[k]:min(off[k] + n[k], ncols)] = 0.0
    elif with_seg_rows:
        seg_rows = [1, 2, 3, 4, 0, 6]
    if nhrows is not None:
        head0 = ints_like((nhrows, NHCOLS), 202, real)
    slabs = [slab_input(t, nslab, real) for t in range(slab_count)]
    sdst0 = [ints_like((32, 32, 3, 3), 220 + t, real) for t in range(slab_count)]
    B = Bufs()
    bsmall, bdst = B.new(small0), [B.new(d) for d in dst0]
    brows = B.new(rows0) if rows0 is not None else None
    bhead = B.new(head0) if head0 is not None else None
    bslab, bsdst = [B.new(s) for s in slabs], [B.new(d) for d in sdst0]
    rc = call("evf_grads_finalize", ptrs(bslab) if slab_count else None, ptrs(bsdst) if slab_count else None, slab_count, nslab,
              bsmall.ptr, clear_small, brows.ptr if brows else None, nrows or 0, ncols if brows else 0,
              bhead.ptr if bhead else None, nhrows or 0, NHCOLS if bhead else 0, HEAD_OFF, ptrs(bdst), ints(off), ints(n),
              ints(seg_rows) if seg_rows is not None else None, nseg)
    assert rc == 0
    ref = R.finalize_ref(slabs, sdst0, small0, clear_small, rows0, head0, HEAD_OFF, dst0, off, n, seg_rows)
    what = f"nrows={nrows} seg_rows={seg_rows} nhrows={nhrows} ncols={ncols} clear_small={clear_small}"
    if real:
        a = R.finalize_ref([np.abs(s) for s in slabs], [np.abs(d) for d in sdst0], np.abs(small0), 0,
                           None if rows0 is None else np.abs(rows0), None if head0 is None else np.abs(head0), HEAD_OFF,
                           [np.abs(d) for d in dst0], off, n, None)
    for k in range(nseg):
        if real:
            assert_close_sum(bdst[k].get(), ref["seg_dst"][k], a["seg_dst"][k], f"segment {k} ({what})")
        else:
            assert_bits(bdst[k].get(), ref["seg_dst"][k], f"evf_grads_finalize segment {k} (off {off[k]}, n {n[k]}; {what})")
    for t in range(slab_count):
        if real:
            assert_close_sum(bsdst[t].get(), ref["slab_dst"][t], a["slab_dst"][t], f"slab tensor {t} ({what})")
        else:
            assert_bits(bsdst[t].get(), ref["slab_dst"][t], f"evf_grads_finalize slab tensor {t} ({what})")
        assert same_bits(bslab[t].get(), slabs[t])
    assert same_bits(bsmall.get(), ref["small"].astype(F32)), f"small: cleared / kept by the flag, nothing else ({what})"
    if brows is not None:
        assert same_bits(brows.get(), ref["rows"].astype(F32)), \
            f"rows: the segments' columns zero up to min(nrows, seg_rows[k]), everything else unchanged ({what})"
    if bhead is not None:
        assert same_bits(bhead.get(), head0), f"head_rows changed ({what})"
    B.check()


@pytest.mark.parametrize("with_seg_rows", (False, True))
@pytest.mark.parametrize("nrows", (1, 255, 256, 257, 700))
def test_grads_finalize_segments(nrows, with_seg_rows):
    """nslabs = 0: the segment part alone.  Sources present and absent, `small` wider than `rows`, clear_small on and off."""
    for nr, nhrows, ncols, clear_small in ((nrows, 300, NSMALL, 1), (nrows, 1, NSMALL, 0), (nrows, None, NSMALL, 1),
                                           (None, 300, NSMALL, 0), (nrows, 1, 230, 1), (None, None, NSMALL, 1)):
        _finalize_case(nr, with_seg_rows, nhrows, ncols, clear_small, real=False)


def test_grads_finalize_slabs_and_segments_in_one_launch():
    _finalize_case(257, True, 300, NSMALL, 1, real=False, slab_count=3, nslab=17)


def test_grads_finalize_real_valued():
    """The longest chain of one output: 257 / 16 rows + 300 / 16 head rows per thread, the 16 row groups, small, dst: 54 <= 64."""
    _finalize_case(257, True, 300, NSMALL, 1, real=True, slab_count=1, nslab=257)


def test_grads_finalize_too_many_segments():
    B = Bufs()
    small0, dst0 = ints_like((NSMALL,), 300), ints_like((4,), 301)
    bsmall, bd = B.new(small0), B.new(dst0)
    off = [4 * k for k in range(33)]
    rc = call("evf_grads_finalize", None, None, 0, 0, bsmall.ptr, 1, None, 0, 0, None, 0, 0, 0, ptrs([bd] * 33), ints(off),
              ints([4] * 33), None, 33)
    assert rc == EINVAL
    assert same_bits(bsmall.get(), small0) and same_bits(bd.get(), dst0)
    B.check()
