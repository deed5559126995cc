"""The zoo's normalisation, element-wise, resampling and concatenation kernels through the C ABI, entry point by entry point,
against the float64 references of tests/zoo_ops_ref.py at the bounds stated there (rule 1: bit for bit; rule 2: an operation
count; rule 3: 4 x a figure measured on the CPU and stored in zoo_ops_ref.MEASURED), which
tests/test_host_zoo_ops_reference.py establishes without a GPU:

evf_chan_reduce (default path), evf_chan_affine, evf_weight_norm_fwd, evf_weight_norm_bwd, evf_act_fwd, evf_act_bwd,
evf_gru_gates_fwd, evf_gru_out_fwd, evf_gru_out_bwd, evf_gru_gates_bwd, evf_lstm_fwd, evf_lstm_bwd, evf_spike_fwd, evf_spike_bwd,
evf_upsample2x_fwd, evf_upsample2x_bwd, evf_upsample_nearest_fwd, evf_upsample_nearest_bwd, evf_concat_channels,
evf_concat_up2_fwd; and hip_ops' batch / instance / group norm end to end against torch's float64 modules.

Every buffer handed to a kernel sits between 64 guard elements on either side (tests/gpu_bufs.py), outputs are pre-filled with
the sentinel, and every case ends with Bufs.check().

EVF_ZOO_OPS_REPORT=<file>: the largest observed error of every output as a fraction of its bound is appended there."""

import ctypes
import os

import numpy as np
import pytest
import torch

import zoo_det_ref as ZD
import zoo_ops_ref as R
from event_flow_amd import _lib
from gpu_bufs import SENTINEL, Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32, F64 = np.float32, np.float64
assert SENTINEL == R.SENTINEL

REPORT = {}


NOTES = ("norm_layers (about 0.01 of the bound): the 256 units are a worst case, 64 rounded operations times a 4-fold amplification by "
         "the variance; the sums have 24 terms of either sign and the observed error is two or three units.",
         "rule 3 outputs sit at 0.25: the kernels reproduce the float32 emulation (the bound is 4 x its error), to the last bits of "
         "the device's tanhf / expf.")


def write_report(title, report, notes=()):
    path = os.environ.get("EVF_ZOO_OPS_REPORT")
    if path and report:
        with open(path, "a") as f:
            f.write(f"{title}: largest error / bound per output (rule 1: bit for bit, 0 = all equal; rule 2: operation count x 2^-24 x "
                    "sum |terms|; rule 3: 4 x the CPU-measured error of the float32 emulation)\n")
            for k, v in sorted(report.items()):
                f.write(f"  {k}: {v:.4f}\n")
            for line in notes:
                f.write(f"  note: {line}\n")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    write_report("tests/test_gpu_zoo_ops.py", REPORT, NOTES)


def call(name, *args):
    return _lib.raw(name, *args)


def ptr(b):
    return None if b is None else b.ptr


def ptrs(bufs):
    return (ctypes.c_void_p * max(len(bufs), 1))(*[ptr(b) for b in bufs])


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])


def new(B, a, shift=0):
    return None if a is None else B.new(a, shift)


def out_buf(B, shape, shift=0):
    return B.new(np.full(shape, SENTINEL, F32), shift)


def judge(family, case, got, report=REPORT):
    """The one assertion of a case: fractions() of the reference module, every output within its bound."""
    exp = R.expect(family, case, R.make(family, case))
    for name, f in R.fractions(exp, got).items():
        key = f"{family}.{name} (rule {exp[name].rule})"
        report[key] = max(report.get(key, 0.0), f)
        assert f <= 1.0, f"{family} {case}: {name} at {f:.3g} of its bound (rule {exp[name].rule})"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32).reshape(a.shape)
    return np.array_equal(a.view(np.int32), b.view(np.int32))


# ============================================================================================================== chan_reduce
def _chan_run(x, y, center, scale, mode, G, npg, C, ld):
    B = Bufs()
    bx, by, bc, bs = B.new(x), B.new(y), B.new(center), B.new(scale)
    out = B.new(np.full((G, C), 7.0e5, F32))  # garbage: the entry point zeroes its output itself
    assert call("evf_chan_reduce", bx.ptr, ld, by.ptr, ld, bc.ptr, bs.ptr, mode, G, npg, C, out.ptr) == 0
    got = out.get()
    B.check()
    assert same_bits(bx.get(), x) and same_bits(by.get(), y)
    return got


@pytest.mark.parametrize("pad", R.CHAN_PADS)
@pytest.mark.parametrize("G,npg,C", R.CHAN_CASES)
def test_chan_reduce_default_path(G, npg, C, pad):
    """Integer-valued inputs (integer center, power-of-two scale): every mode bit for bit whatever order the atomics land in.
    Real inputs: rule 2 with k = the mode's operations + npg summed terms."""
    x, y, center, scale = R.chan_int_inputs(G, npg, C, pad)
    for mode in range(3):
        ref, _ = ZD.chan_ref64(x, y, center, scale, mode, G, npg, C)
        got = _chan_run(x, y, center, scale, mode, G, npg, C, C + pad)
        ok = R.bits_equal(got, ref)
        assert ok.all(), f"mode {mode}: {(~ok).sum()} sums differ, first {got[~ok][0]} != {ref[~ok][0]}"
    x, y, center, scale, _ = ZD.chan_inputs(G, npg, C, pad)
    for mode in range(3):
        ref, sabs = ZD.chan_ref64(x, y, center, scale, mode, G, npg, C)
        got = _chan_run(x, y, center, scale, mode, G, npg, C, C + pad)
        f = float(np.max(np.abs(got.astype(F64) - ref) / ((R.K2["chan_reduce"][mode] + npg) * R.U * sabs)))
        key = f"chan_reduce.mode{mode} (rule 2)"
        REPORT[key] = max(REPORT.get(key, 0.0), f)
        assert f <= 1.0, (mode, f)


def test_chan_reduce_refusals():
    B = Bufs()
    x, y, center, scale = R.chan_int_inputs(1, 5, 3, 0)
    bx, by, out = B.new(x), B.new(y), out_buf(B, (1, 3))
    for args in ((None, 3, by.ptr, 3, None, None, 0, 1, 5, 3, out.ptr), (bx.ptr, 2, by.ptr, 3, None, None, 0, 1, 5, 3, out.ptr),
                 (bx.ptr, 3, None, 3, None, None, 2, 1, 5, 3, out.ptr), (bx.ptr, 3, by.ptr, 2, None, None, 2, 1, 5, 3, out.ptr),
                 (bx.ptr, 3, by.ptr, 3, None, None, 3, 1, 5, 3, out.ptr), (bx.ptr, 3, by.ptr, 3, None, None, 0, 0, 5, 3, out.ptr),
                 (bx.ptr, 3, by.ptr, 3, None, None, 0, 1, 0, 3, out.ptr), (bx.ptr, 3, by.ptr, 3, None, None, 0, 1, 5, 3, None)):
        assert call("evf_chan_reduce", *args) == EINVAL
    assert (out.get() == SENTINEL).all()
    B.check()


# ============================================================================================================== chan_affine
@pytest.mark.parametrize("case", R.AFFINE_CASES)
def test_chan_affine(case):
    """Forward form (g null) and backward form; ldg, ldx, ldo all different and larger than C: the padding columns of `out` keep
    the sentinel.  Bit for bit against the float32 emulation (no contraction), rule 2 with k = 4 against float64."""
    G, npg, C, bwd = case
    i = R.make("chan_affine", case)
    B = Bufs()
    bg, bx, bA, bB, bC = new(B, i["g"]), B.new(i["x"]), B.new(i["A"]), B.new(i["Bc"]), B.new(i["Cc"])
    out = out_buf(B, (G * npg, i["ldo"]))
    assert call("evf_chan_affine", ptr(bg), i["ldg"], bx.ptr, i["ldx"], bA.ptr if bwd else None, bB.ptr, bC.ptr, G, npg, C, out.ptr,
                i["ldo"]) == 0
    got = out.get()
    B.check()
    judge("chan_affine", case, {"out": got})
    assert same_bits(got, R.run("chan_affine", case, i, F32)["out"]), "not the float32 expression (a contraction?)"
    assert (got[:, C:] == SENTINEL).all()


def test_chan_affine_refusals():
    case = (1, 7, 3, 1)
    i = R.make("chan_affine", case)
    B = Bufs()
    bg, bx, bA, bB, bC = B.new(i["g"]), B.new(i["x"]), B.new(i["A"]), B.new(i["Bc"]), B.new(i["Cc"])
    out = out_buf(B, (7, i["ldo"]))
    ok = [bg.ptr, i["ldg"], bx.ptr, i["ldx"], bA.ptr, bB.ptr, bC.ptr, 1, 7, 3, out.ptr, i["ldo"]]
    for k, v in ((2, None), (5, None), (6, None), (10, None), (4, None), (1, 2), (3, 2), (11, 2), (7, 0), (8, 0), (9, 0)):
        a = list(ok)
        a[k] = v
        assert call("evf_chan_affine", *a) == EINVAL, k
    assert (out.get() == SENTINEL).all()
    B.check()


# =============================================================================================================== weight norm
@pytest.mark.parametrize("case", R.WN_CASES, ids=str)
def test_weight_norm(case):
    """Forward (w and nrm) and backward (gv, gg) against float64 torch.nn.utils.weight_norm semantics.  Rows scaled by 1e-18 and
    1e+18: the float64 values wherever the float32 sum of squares is finite; where it overflows, torch's own float32 result
    (nrm = inf, w = 0, zero gradients).  The backward once formed g <gw, v> / nrm^3, which under- / overflows for those rows
    (inf / NaN gradients for the 1e-18 row, the projection term lost for a finite 1e+18 row): it now divides by nrm^2 as
    ATen does."""
    Cout, n = case
    i = R.make("wn_bwd", case)
    B = Bufs()
    bv, bg, bgw, bn = B.new(i["v"]), B.new(i["g"]), B.new(i["gw"]), B.new(i["nrm"])
    w, nrm, gv, gg = out_buf(B, (Cout, n)), out_buf(B, (Cout,)), out_buf(B, (Cout, n)), out_buf(B, (Cout,))
    assert call("evf_weight_norm_fwd", bv.ptr, bg.ptr, Cout, n, w.ptr, nrm.ptr) == 0
    assert call("evf_weight_norm_bwd", bgw.ptr, bv.ptr, bg.ptr, bn.ptr, Cout, n, gv.ptr, gg.ptr) == 0
    got = {"w": w.get(), "nrm": nrm.get(), "gv": gv.get(), "gg": gg.get()}
    B.check()
    judge("wn_fwd", case, got)
    judge("wn_bwd", case, got)
    assert call("evf_weight_norm_fwd", bv.ptr, bg.ptr, 0, n, w.ptr, nrm.ptr) == EINVAL
    assert call("evf_weight_norm_bwd", bgw.ptr, bv.ptr, bg.ptr, None, Cout, n, gv.ptr, gg.ptr) == EINVAL


# =============================================================================================================== activations
@pytest.mark.parametrize("case", R.ACT_CASES, ids=str)
def test_activations(case):
    """kind 0 - 3, with and without residual, into a buffer of its own and with y aliasing x; the backward through the output."""
    kind, res, n = case
    i = R.make("act_bwd", case)
    B = Bufs()
    bx, br, by, bgy = B.new(i["x"]), new(B, i["r"]), B.new(i["y"]), B.new(i["gy"])
    y, gx = out_buf(B, (n,)), out_buf(B, (n,))
    assert call("evf_act_fwd", kind, bx.ptr, ptr(br), n, y.ptr) == 0
    judge("act_fwd", case, {"y": y.get()})
    assert same_bits(bx.get(), i["x"])
    assert call("evf_act_fwd", kind, bx.ptr, ptr(br), n, bx.ptr) == 0  # in place
    assert same_bits(bx.get(), y.get()), "y aliasing x gives other bits"
    assert call("evf_act_bwd", kind, by.ptr, bgy.ptr, n, gx.ptr) == 0
    judge("act_bwd", case, {"gx": gx.get()})
    B.check()


def test_activation_refusals():
    B = Bufs()
    x, y = B.new(np.ones(4, F32)), out_buf(B, (4,))
    for kind in (4, -1):
        assert call("evf_act_fwd", kind, x.ptr, None, 4, y.ptr) == EINVAL
        assert call("evf_act_bwd", kind, x.ptr, x.ptr, 4, y.ptr) == EINVAL
    assert call("evf_act_fwd", 1, x.ptr, None, 0, y.ptr) == EINVAL
    assert (y.get() == SENTINEL).all()
    B.check()


# ======================================================================================================================= GRU
@pytest.mark.parametrize("case", R.GRU_CASES, ids=str)
def test_gru_entry_points_one_by_one(case):
    """h null (the first step) and given; evf_gru_out_bwd must OVERWRITE g_h (pre-filled with the sentinel), evf_gru_gates_bwd must
    ADD onto it."""
    n, has_h = case
    i = R.make("gru_chain", case)
    B = Bufs()
    b = {k: new(B, i[k]) for k in ("cu", "cr", "co", "h", "u", "r", "o", "g_new", "g_hr")}
    o = {k: out_buf(B, (n,)) for k in ("u", "r", "hr", "o", "hn", "g_co", "g_cu", "g_h", "g_cr")}
    gh0 = B.new(i["g_h0"])
    assert call("evf_gru_gates_fwd", b["cu"].ptr, b["cr"].ptr, ptr(b["h"]), n, o["u"].ptr, o["r"].ptr, o["hr"].ptr) == 0
    judge("gru_gates_fwd", case, {k: o[k].get() for k in ("u", "r", "hr")})
    assert call("evf_gru_out_fwd", b["co"].ptr, ptr(b["h"]), b["u"].ptr, n, o["o"].ptr, o["hn"].ptr) == 0
    judge("gru_out_fwd", case, {k: o[k].get() for k in ("o", "hn")})
    assert call("evf_gru_out_bwd", b["g_new"].ptr, ptr(b["h"]), b["u"].ptr, b["o"].ptr, n, o["g_co"].ptr, o["g_cu"].ptr, o["g_h"].ptr) == 0
    judge("gru_out_bwd", case, {k: o[k].get() for k in ("g_co", "g_cu", "g_h")})
    assert call("evf_gru_gates_bwd", b["g_hr"].ptr, ptr(b["h"]), b["r"].ptr, n, o["g_cr"].ptr, gh0.ptr) == 0
    judge("gru_gates_bwd", case, {"g_cr": o["g_cr"].get(), "g_h": gh0.get()})
    for k in ("cu", "cr", "co", "u", "r", "o", "g_new", "g_hr"):
        assert same_bits(b[k].get(), i[k]), k
    B.check()


@pytest.mark.parametrize("case", R.GRU_CASES, ids=str)
def test_gru_entry_points_chained_against_autograd(case):
    """The four in the order of a step (the out-gate convolution stood in for by co = c0 + kk * hr on the host) against the float64
    gradients of submodules.py:412-416, which tests/test_host_zoo_ops_reference.py checks against autograd."""
    n, has_h = case
    i = R.make("gru_chain", case)
    B = Bufs()
    cu, cr, h, g_new = B.new(i["cu"]), B.new(i["cr"]), new(B, i["h"]), B.new(i["g_new"])
    u, r, hr, o, hn, g_co, g_cu, g_h, g_cr = (out_buf(B, (n,)) for _ in range(9))
    assert call("evf_gru_gates_fwd", cu.ptr, cr.ptr, ptr(h), n, u.ptr, r.ptr, hr.ptr) == 0
    co = B.new((i["c0"] + (i["kk"] * hr.get()).astype(F32)).astype(F32))
    assert call("evf_gru_out_fwd", co.ptr, ptr(h), u.ptr, n, o.ptr, hn.ptr) == 0
    assert call("evf_gru_out_bwd", g_new.ptr, ptr(h), u.ptr, o.ptr, n, g_co.ptr, g_cu.ptr, g_h.ptr) == 0
    g_hr = B.new((i["kk"] * g_co.get()).astype(F32))
    assert call("evf_gru_gates_bwd", g_hr.ptr, ptr(h), r.ptr, n, g_cr.ptr, g_h.ptr) == 0
    judge("gru_chain", case, {"hn": hn.get(), "g_co": g_co.get(), "g_cu": g_cu.get(), "g_cr": g_cr.get(), "g_h": g_h.get()})
    B.check()


def test_gru_refusals():
    B = Bufs()
    x, y = B.new(np.ones(4, F32)), out_buf(B, (4,))
    assert call("evf_gru_gates_fwd", None, x.ptr, None, 4, y.ptr, y.ptr, y.ptr) == EINVAL
    assert call("evf_gru_out_fwd", x.ptr, None, None, 4, y.ptr, y.ptr) == EINVAL
    assert call("evf_gru_out_bwd", x.ptr, None, x.ptr, x.ptr, 0, y.ptr, y.ptr, y.ptr) == EINVAL
    assert call("evf_gru_gates_bwd", x.ptr, None, None, 4, y.ptr, y.ptr) == EINVAL
    assert (y.get() == SENTINEL).all()
    B.check()


# ====================================================================================================================== LSTM
@pytest.mark.parametrize("case", R.LSTM_CASES, ids=str)
def test_lstm(case):
    """prev_cell null and given; the forward overwrites `gates` in place with the activated values; in the backward each of
    g_hidden / g_cell / g_prev_cell null in turn, and g_hidden and g_cell both null refused."""
    Ch, npix, pc, miss = case
    i = R.make("lstm_bwd", case)
    B = Bufs()
    if miss == "none":
        gates, prev = B.new(i["gates"]), new(B, i["prev_cell"])
        cell, hidden = out_buf(B, (npix, Ch)), out_buf(B, (npix, Ch))
        assert call("evf_lstm_fwd", gates.ptr, ptr(prev), npix, Ch, cell.ptr, hidden.ptr) == 0
        judge("lstm_fwd", case, {"gates": gates.get(), "cell": cell.get(), "hidden": hidden.get()})
    act, cl, prev = B.new(i["act"]), B.new(i["cell"]), new(B, i["prev_cell"])
    gh, gc = new(B, i["g_hidden"]), new(B, i["g_cell"])
    gg = out_buf(B, (npix, 4 * Ch))
    gp = None if miss == "g_prev_cell" else out_buf(B, (npix, Ch))
    assert call("evf_lstm_bwd", ptr(gh), ptr(gc), act.ptr, cl.ptr, ptr(prev), npix, Ch, gg.ptr, ptr(gp)) == 0
    got = {"g_gates": gg.get()}
    if gp is not None:
        got["g_prev_cell"] = gp.get()
    judge("lstm_bwd", case, got)
    assert same_bits(act.get(), i["act"]) and same_bits(cl.get(), i["cell"])
    assert call("evf_lstm_bwd", None, None, act.ptr, cl.ptr, ptr(prev), npix, Ch, gg.ptr, ptr(gp)) == EINVAL
    assert call("evf_lstm_fwd", act.ptr, None, npix, 0, cl.ptr, cl.ptr) == EINVAL
    assert same_bits(gg.get(), got["g_gates"])
    B.check()


# ==================================================================================================================== spikes
@pytest.mark.parametrize("case", R.SPIKE_CASES, ids=str)
def test_spike_functions(case):
    """The four surrogates, scalar and per-element threshold, inputs at exactly the threshold and one ulp either side: the forward
    bit for bit."""
    s, per, n = case
    i = R.make("spike_bwd", case)
    B = Bufs()
    x, th, g = B.new(i["x"]), B.new(i["th"]), B.new(i["g"])
    z, gx = out_buf(B, (n,)), out_buf(B, (n,))
    assert call("evf_spike_fwd", x.ptr, th.ptr, per, n, z.ptr) == 0
    judge("spike_fwd", (0, per, n), {"z": z.get()})
    assert call("evf_spike_bwd", s, x.ptr, th.ptr, per, g.ptr, float(R.SPIKE_WIDTH[s]), n, gx.ptr) == 0
    judge("spike_bwd", case, {"gx": gx.get()})
    assert call("evf_spike_bwd", 4, x.ptr, th.ptr, per, g.ptr, 1.0, n, gx.ptr) == EINVAL
    assert call("evf_spike_fwd", x.ptr, None, per, n, z.ptr) == EINVAL
    B.check()


# ================================================================================================================ resampling
@pytest.mark.parametrize("case", R.UP2_CASES, ids=str)
def test_upsample2x(case):
    """Every one of the three vector widths, reached by divisibility of C and by the alignment of both pointers (shifted by 0, 1
    and 2 floats); H = 1 / W = 1 make every tap a border tap.  Integer inputs: forward and exact transpose bit for bit."""
    Bn, H, W, C, shift = case
    i = R.make("up2_fwd", case)
    B = Bufs()
    x, gy = B.new(i["x"], shift), B.new(i["gy"], shift)
    y, gx = out_buf(B, (Bn, 2 * H, 2 * W, C), shift), out_buf(B, (Bn, H, W, C), shift)
    assert call("evf_upsample2x_fwd", x.ptr, Bn, H, W, C, y.ptr) == 0
    assert call("evf_upsample2x_bwd", gy.ptr, Bn, H, W, C, gx.ptr) == 0
    judge("up2_fwd", case, {"y": y.get()})
    judge("up2_bwd", case, {"gx": gx.get()})
    B.check()
    if shift == 0 and C % 4 == 0:  # an aligned input with a misaligned output must leave the vector path as well
        y1 = out_buf(B, (Bn, 2 * H, 2 * W, C), 1)
        assert call("evf_upsample2x_fwd", x.ptr, Bn, H, W, C, y1.ptr) == 0
        judge("up2_fwd", case, {"y": y1.get()})
        B.check()
    assert call("evf_upsample2x_fwd", x.ptr, Bn, H, 0, C, y.ptr) == EINVAL
    assert call("evf_upsample2x_bwd", None, Bn, H, W, C, gx.ptr) == EINVAL


@pytest.mark.parametrize("case", R.NEAR_CASES, ids=str)
def test_upsample_nearest(case):
    planes, h, w, f = case
    i = R.make("near_fwd", case)
    B = Bufs()
    x, gy = B.new(i["x"]), B.new(i["gy"])
    y, gx = out_buf(B, (planes, h * f, w * f)), out_buf(B, (planes, h, w))
    assert call("evf_upsample_nearest_fwd", x.ptr, planes, h, w, f, y.ptr) == 0
    assert call("evf_upsample_nearest_bwd", gy.ptr, planes, h, w, f, gx.ptr) == 0
    judge("near_fwd", case, {"y": y.get()})
    judge("near_bwd", case, {"gx": gx.get()})
    assert call("evf_upsample_nearest_fwd", x.ptr, planes, h, w, 0, y.ptr) == EINVAL
    assert call("evf_upsample_nearest_bwd", gy.ptr, 0, h, w, f, gx.ptr) == EINVAL
    B.check()


# ============================================================================================================ concatenation
def _part_args(B, chans, parts):
    bufs = [new(B, p) for p in parts]
    C = [c for c, _ in chans]
    ld = [c if p is None else p.shape[1] for c, p in zip(C, parts)]
    return bufs, C, ld


@pytest.mark.parametrize("case", R.CASES["concat"], ids=str)
def test_concat_channels(case):
    """1, 3 and 6 parts, odd channel counts, a null part in the middle and at the end (zeros), part strides larger than their
    channels, ldo larger than the total: the padding keeps the sentinel."""
    (chans, pad, opad), npix = case
    i = R.make("concat", case)
    B = Bufs()
    bufs, C, ld = _part_args(B, chans, i["parts"])
    tot = sum(C)
    out = out_buf(B, (npix, tot + opad))
    assert call("evf_concat_channels", ptrs(bufs), ints(C), ints(ld), len(C), npix, out.ptr, tot + opad) == 0
    judge("concat", case, {"out": out.get()})
    for b, p in zip(bufs, i["parts"]):
        assert b is None or same_bits(b.get(), p)
    B.check()


def test_concat_channels_refusals():
    case = R.CASES["concat"][6]  # three parts
    (chans, pad, opad), npix = case
    i = R.make("concat", case)
    B = Bufs()
    bufs, C, ld = _part_args(B, chans, i["parts"])
    tot = sum(C)
    out = out_buf(B, (npix, tot + opad))
    seven = ((bufs * 7)[:7], (C * 7)[:7], (ld * 7)[:7])
    assert call("evf_concat_channels", ptrs(seven[0]), ints(seven[1]), ints(seven[2]), 7, npix, out.ptr, 64) == EINVAL
    assert call("evf_concat_channels", ptrs(bufs), ints(C), ints(ld), 0, npix, out.ptr, tot + opad) == EINVAL
    for bad in (0, -1):
        assert call("evf_concat_channels", ptrs(bufs), ints([C[0], bad, C[2]]), ints(ld), 3, npix, out.ptr, tot + opad) == EINVAL
    assert call("evf_concat_channels", ptrs(bufs), ints(C), ints([ld[0], C[1] - 1, ld[2]]), 3, npix, out.ptr, tot + opad) == EINVAL
    assert call("evf_concat_channels", ptrs(bufs), ints(C), ints(ld), 3, npix, out.ptr, tot - 1) == EINVAL
    assert call("evf_concat_channels", ptrs(bufs), ints(C), ints(ld), 3, 0, out.ptr, tot + opad) == EINVAL
    assert (out.get() == SENTINEL).all()
    B.check()


@pytest.mark.parametrize("case", R.CUP_CASES, ids=str)
def test_concat_up2(case):
    """upsample(concat) in one kernel against the float64 composition, bit for bit on integer inputs: channel quads that straddle
    two parts and a part and the zero padding, every border shape, strided parts, a padded output."""
    chans, Bn, H, W, pad = case
    i = R.make("concat_up2", case)
    B = Bufs()
    bufs, C, ld = _part_args(B, chans, i["parts"])
    tot = sum(C)
    out = out_buf(B, (Bn, 2 * H, 2 * W, tot + 4))
    assert call("evf_concat_up2_fwd", ptrs(bufs), ints(C), ints(ld), len(C), Bn, H, W, out.ptr, tot + 4) == 0
    judge("concat_up2", case, {"out": out.get()})
    B.check()


def test_concat_up2_refusals():
    """Every precondition in the comment above the entry point."""
    B = Bufs()
    H = W = 3
    a = B.new(np.ones((H * W, 6), F32))
    b = B.new(np.ones((H * W, 6), F32))
    odd = B.new(np.ones((H * W, 6), F32), shift=1)  # 4-byte aligned only
    out = out_buf(B, (2 * H, 2 * W, 16))
    out_odd = out_buf(B, (2 * H, 2 * W, 16), shift=2)  # 8-byte aligned only

    def run(src, C, ld, o=out, ldo=12):
        return call("evf_concat_up2_fwd", ptrs(src), ints(C), ints(ld), len(C), 1, H, W, o.ptr, ldo)

    assert run([a, b], [3, 5], [6, 6]) == EINVAL  # odd C
    assert run([a, b], [2, 2], [5, 6]) == EINVAL  # odd ld
    assert run([a, b], [2, 4], [6, 6]) == EINVAL  # total 6: not a multiple of 4
    assert run([a, b], [2, 2], [6, 6], ldo=6) == EINVAL  # ldo & 3
    assert run([a, b], [2, 2], [6, 6], o=out_odd) == EINVAL  # misaligned out
    assert run([a, odd], [2, 2], [6, 6]) == EINVAL  # misaligned part
    assert run([None, b], [2, 2], [6, 6]) == EINVAL  # null first part
    assert run([a, b], [2, 2], [6, 1]) == EINVAL  # ld < C
    assert run([a, b], [4, 4], [6, 6], ldo=4) == EINVAL  # ldo < total
    assert (out.get() == SENTINEL).all() and (out_odd.get() == SENTINEL).all()
    assert run([a, b], [2, 2], [6, 6]) == 0
    B.check()


# ================================================================================================= norms end to end (hip_ops)
NORM_TOL = 256  # units of 2^-24 * max(1, |ref|), see test_norm_layers_end_to_end


@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("kind", ("batch", "instance", "group"))
def test_norm_layers_end_to_end(kind, train):
    """hip_ops.norm2d / group_norm1 forward and backward at B = 2, C = 5, 3 x 4 against torch's float64 modules and autograd, the
    running statistics too.  Tolerance 256 units of 2^-24 * max(1, |ref|): every output is reached from the inputs through
    fewer than 64 rounded operations (two sums of <= 24 terms, the host's coefficient arithmetic, the affine pass), each of which
    errs by 2^-24 of a quantity that the variance of these inputs (>= 0.25 per statistic, asserted) amplifies at most 4-fold."""
    from event_flow_amd.models import hip_ops

    rng = np.random.default_rng(17)
    x0 = rng.normal(0.3, 1.0, (2, 5, 3, 4))
    gy0 = rng.normal(0, 1, (2, 5, 3, 4))
    make = {"batch": lambda: torch.nn.BatchNorm2d(5), "instance": lambda: torch.nn.InstanceNorm2d(5, affine=True, track_running_stats=True),
            "group": lambda: torch.nn.GroupNorm(1, 5)}[kind]
    ref = make().double()
    with torch.no_grad():
        ref.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, 5)))
        ref.bias.copy_(torch.from_numpy(rng.normal(0, 0.5, 5)))
        if kind != "group":
            ref.running_mean.copy_(torch.from_numpy(rng.normal(0.3, 0.2, 5)))
            ref.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, 5)))
    var = {"batch": x0.var((0, 2, 3)), "instance": x0.var((2, 3)), "group": x0.var((1, 2, 3))}[kind]
    assert var.min() >= 0.25
    mine = make().float()
    mine.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    mine = mine.to(DEV)
    ref.train(train), mine.train(train)
    xr = torch.from_numpy(x0).requires_grad_()
    yr = ref(xr)
    yr.backward(torch.from_numpy(gy0))
    xm = torch.from_numpy(x0.astype(F32)).to(DEV).requires_grad_()
    ym = hip_ops.group_norm1(xm, mine) if kind == "group" else hip_ops.norm2d(xm, mine)
    ym.backward(torch.from_numpy(gy0.astype(F32)).to(DEV))
    pairs = [("y", ym, yr), ("g_x", xm.grad, xr.grad), ("g_weight", mine.weight.grad, ref.weight.grad),
             ("g_bias", mine.bias.grad, ref.bias.grad)]
    if kind != "group":
        pairs += [("running_mean", mine.running_mean, ref.running_mean), ("running_var", mine.running_var, ref.running_var)]
    for name, a, b in pairs:
        a, b = a.detach().cpu().double().numpy(), b.detach().numpy()
        f = float(np.max(np.abs(a - b)) / (NORM_TOL * R.U * max(1.0, float(np.max(np.abs(b))))))
        key = f"norm_layers.{name} (256 units)"
        REPORT[key] = max(REPORT.get(key, 0.0), f)
        assert f <= 1.0, (kind, train, name, f)
