"""Deterministic mode for voxel-input fused FireNets and norm_input: evf_head_wgrad_det, evf_lif_bwd_det and
evf_norm_nonzero_det through the C ABI against the float64 references of tests/head_det_ref.py at the bounds derived there, bit
for bit from call to call, from NaN-filled scratch and from a captured hipGraph; the engine's and hip_ops' routing behind
EVF_DETERMINISTIC / set_deterministic; and whole voxel-input training steps repeated bit for bit through the real loss.

EVF_DET_VOXEL_REPORT=<file>: the largest observed error of every regime as a fraction of its bound is written there."""

import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_det_ref as HD
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
F32, F64 = np.float32, np.float64
FILL = 7.0  # initial contents of outputs that a kernel must overwrite (or must leave alone)
C = HD.C

REPORT = {}  # regime -> {output: fraction of its bound}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("EVF_DET_VOXEL_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("bounds in units of 2^-24 * sum |terms| (tests/head_det_ref.py): head weight gradient 1 + chain; g_leak / g_thresh "
                    f"ops ({HD.lif_ops(np.exp(HD.LEAK_MAX))['leak']:.1f} / {HD.lif_ops(0)['thresh']}) + chain; norm_input {HD.NORM_OPS}\n")
            for regime, r in REPORT.items():
                f.write(f"{regime}: error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(r.items())) + "\n")


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def call(name, *args):
    return _lib.raw(name, *args)


def P(b):
    return None if b is None else b.ptr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def within(regime, name, got, ref, scale, k):
    """|got - ref| <= k * 2^-24 * scale everywhere (equal non-finite patterns); prints and records the fraction of the bound used."""
    worst = HD.units(got, ref, scale) / k
    print(f"  {regime} {name}: {worst:.3f} of the bound ({k:.1f} units)")
    r = REPORT.setdefault(regime, {})
    r[name] = max(r.get(name, 0.0), float(worst))
    assert worst <= 1.0, f"{regime} {name}: {worst:.3f} of the bound"


def sum_rows(B, rows, nrows, n):
    """evf_sum_rows(accumulate = 0) over a [nrows][n] buffer -> [n] (into a FILL-ed output: it must overwrite)."""
    dst = B.new(np.full(n, FILL, F32))
    assert call("evf_sum_rows", rows.ptr, nrows, n, 0, dst.ptr) == 0
    torch.cuda.synchronize()
    return dst.get()


# ================================================================================================================ head wgrad
def head_call(x, g, case, slab, acc, name="evf_head_wgrad_det"):
    Bn, Cin, H, W = case
    if name == "evf_head_wgrad":
        return call(name, x.ptr, g.ptr, Bn, Cin, H, W, slab.ptr)
    return call(name, P(x), P(g), Bn, Cin, H, W, P(slab), acc)


@pytest.mark.parametrize("case", HD.HEAD_CASES)
def test_head_wgrad_det(case):
    """Exact leg: integer data, slab rows summed by evf_sum_rows equal the integer reference, a second accumulating call on fresh
    data the sum of both.  Real leg: float64 at the derived bound, two calls and a NaN-filled against a random slab the same bits,
    the default entry point inside the same bound."""
    L = _lib.load()
    B = Bufs()
    Bn, Cin, H, W = case
    nsl, n = L.evf_head_wgrad_det_slabs(Bn, H, W), C * Cin * 9
    assert nsl == HD.head_wgrad_det_slabs(Bn, H, W)
    regime = f"head_wgrad {case}"
    # ---- exact
    x0, g0 = HD.head_inputs(case, "exact", 0)
    x1, g1 = HD.head_inputs(case, "exact", 1)
    r0, r1 = HD.head_wgrad_ref64(x0, g0)[0], HD.head_wgrad_ref64(x1, g1)[0]
    xb, gb = B.new(x0), B.new(g0)
    slab = B.new(np.random.default_rng(1).normal(0, 1e3, (nsl, n)))  # (need not be zero on entry)
    assert head_call(xb, gb, case, slab, 0) == 0
    assert np.array_equal(sum_rows(B, slab, nsl, n).reshape(r0.shape).astype(F64), r0)
    xb.set(x1), gb.set(g1)
    assert head_call(xb, gb, case, slab, 1) == 0
    assert np.array_equal(sum_rows(B, slab, nsl, n).reshape(r0.shape).astype(F64), r0 + r1)
    # ---- real
    x, g = HD.head_inputs(case, "real")
    ref, scale = HD.head_wgrad_ref64(x, g)
    xb.set(x), gb.set(g)
    assert head_call(xb, gb, case, slab, 0) == 0
    torch.cuda.synchronize()
    rows_a = slab.get()
    got = sum_rows(B, slab, nsl, n).reshape(ref.shape)
    within(regime, "dw", got, ref, scale, HD.head_bound(*case))
    slab.set(np.full((nsl, n), np.nan, F32))
    assert head_call(xb, gb, case, slab, 0) == 0
    torch.cuda.synchronize()
    assert same_bits(slab.get(), rows_a), "a NaN-filled slab and a random one give different rows"
    assert head_call(xb, gb, case, slab, 0) == 0
    torch.cuda.synchronize()
    assert same_bits(slab.get(), rows_a) and same_bits(sum_rows(B, slab, nsl, n).reshape(ref.shape), got)
    dense = B.new(np.zeros(n, F32))
    assert head_call(xb, gb, case, dense, 0, "evf_head_wgrad") == 0
    torch.cuda.synchronize()
    within(regime, "dw (default entry)", dense.get().reshape(ref.shape), ref, scale, HD.head_bound(*case))
    B.check()


def test_head_wgrad_det_refusals():
    B = Bufs()
    case = HD.HEAD_CASES[1]
    x, g = HD.head_inputs(case, "real")
    big = np.zeros((2, 9, 5, 8), F32)
    xb, gb, xbig = B.new(x), B.new(g), B.new(big)
    slab = B.new(np.full((2, C * 9 * 9), FILL, F32))
    assert head_call(xbig, gb, (2, 9, 5, 8), slab, 0) == EINVAL
    assert head_call(xb, gb, (2, 0, 5, 8), slab, 0) == EINVAL
    assert head_call(xb, gb, case, None, 0) == EINVAL
    assert head_call(None, gb, case, slab, 0) == EINVAL and head_call(xb, None, case, slab, 0) == EINVAL
    torch.cuda.synchronize()
    assert np.all(slab.get() == FILL)
    B.check()


# ================================================================================================================ lif backward
ROW_LD, COL_LEAK, COL_THRESH = 80, 3, 40  # the rows buffer: a pitch wider than the 64 columns, the two outputs apart


def lif_bufs(B, d, npix):
    nb = lambda a: None if a is None else B.new(a)  # noqa: E731
    return {"g_z": nb(d["g_z"]), "g_v": nb(d["g_v"]), "v_out": B.new(d["v_out"]), "v_prev": nb(d["v_prev"]),
            "z_prev": None if d["z_prev"] is None else B.new(d["z_prev"].view(F32)),  # (bit patterns; copied, never converted)
            "leak": B.new(d["leak"]), "thresh": B.new(d["thresh"]),
            "g_cur": B.new(np.full((npix, C), FILL, F32)), "g_v_prev": B.new(np.full((npix, C), FILL, F32))}


def lif_call(b, case, hard, surrogate, rows=None, dense=None, row_ld=ROW_LD, nrows=None):
    Bn, H, W, nr = case
    head = (P(b["g_z"]), P(b["g_v"]), b["v_out"].ptr, P(b["v_prev"]), P(b["z_prev"]), b["leak"].ptr, b["thresh"].ptr, Bn, H, W,
            1 if hard else 0, surrogate, HD.WIDTH[surrogate], b["g_cur"].ptr, b["g_v_prev"].ptr)
    if rows is None:
        return call("evf_lif_bwd", *head, dense[0].ptr, dense[1].ptr)
    return call("evf_lif_bwd_det", *head, rows.ptr + 4 * COL_LEAK, rows.ptr + 4 * COL_THRESH, row_ld, nr if nrows is None else nrows)


@pytest.mark.parametrize("case", HD.LIF_CASES)
def test_lif_bwd_det(case):
    """Hard and soft reset, arctan and superspike, the first-pass nulls and a null g_z: g_cur / g_v_prev are the default entry
    point's bits; the row sums against float64 at the derived bound, the floor channel's g_thresh exactly 0; two calls from
    zeroed rows the same bits; rows behind the grid and columns outside the 64 untouched; the default's dense sums in the bound."""
    Bn, H, W, nrows = case
    npix = Bn * H * W
    nblk = HD.lif_bwd_grid(Bn, H, W, nrows)
    variants = [(hard, sg, "full") for hard in (True, False) for sg in (HD.ARCTAN, HD.SUPERSPIKE)]
    variants += [(True, HD.ARCTAN, "first"), (False, HD.SUPERSPIKE, "first"), (True, HD.ARCTAN, "no g_z")]
    for hard, sg, mode in variants:
        B = Bufs()
        d = HD.lif_inputs(case, first=mode == "first")
        if mode == "no g_z":
            d["g_z"] = None
        b = lif_bufs(B, d, npix)
        r = HD.lif_bwd_ref64(d, hard, sg, nblk)
        regime = f"lif_bwd {case} {'hard' if hard else 'soft'} {'arctan' if sg == HD.ARCTAN else 'superspike'} {mode}"
        # rows: zero where the grid writes, FILL behind it
        init = np.zeros((nrows, ROW_LD), F32)
        init[nblk:] = FILL
        init[:, :COL_LEAK] = init[:, COL_LEAK + C:COL_THRESH] = init[:, COL_THRESH + C:] = FILL
        rows = B.new(init)
        assert lif_call(b, case, hard, sg, rows) == 0
        torch.cuda.synchronize()
        got_rows, g_cur, g_vp = rows.get(), b["g_cur"].get(), b["g_v_prev"].get()
        keep = np.ones_like(init, bool)
        keep[:nblk, COL_LEAK:COL_LEAK + C] = keep[:nblk, COL_THRESH:COL_THRESH + C] = False
        assert np.array_equal(got_rows[keep], init[keep]), "rows behind the grid or columns outside the outputs were written"
        assert not np.any(g_cur == FILL) and not np.any(g_vp == FILL)
        # the default entry point on the same inputs: the same element-wise bits, dense sums inside the same bound
        dense = (B.new(np.zeros(C, F32)), B.new(np.zeros(C, F32)))
        assert lif_call(b, case, hard, sg, dense=dense) == 0
        torch.cuda.synchronize()
        assert same_bits(b["g_cur"].get(), g_cur) and same_bits(b["g_v_prev"].get(), g_vp)
        # sums from all-zero rows
        rows.set(np.zeros((nrows, ROW_LD), F32))
        assert lif_call(b, case, hard, sg, rows) == 0
        torch.cuda.synchronize()
        rows_a = rows.get()
        tot = sum_rows(B, rows, nrows, ROW_LD)
        g_leak, g_thresh = tot[COL_LEAK:COL_LEAK + C], tot[COL_THRESH:COL_THRESH + C]
        kl, kt = HD.lif_bound(case, "leak"), HD.lif_bound(case, "thresh")
        within(regime, "g_leak", g_leak, r["g_leak"], r["scale_leak"], kl)
        within(regime, "g_thresh", g_thresh, r["g_thresh"], r["scale_thresh"], kt)
        assert g_thresh[HD.THRESH_FLOOR_CHANNEL] == 0.0 and np.all(rows_a[:, COL_THRESH + HD.THRESH_FLOOR_CHANNEL] == 0.0)
        assert np.array_equal(g_thresh == 0, r["g_thresh"] == 0) and np.array_equal(g_leak == 0, r["g_leak"] == 0)
        within(regime, "g_leak (default entry)", dense[0].get(), r["g_leak"], r["scale_leak"], kl)
        within(regime, "g_thresh (default entry)", dense[1].get(), r["g_thresh"], r["scale_thresh"], kt)
        assert dense[1].get()[HD.THRESH_FLOOR_CHANNEL] == 0.0
        rows.set(np.zeros((nrows, ROW_LD), F32))
        assert lif_call(b, case, hard, sg, rows) == 0
        torch.cuda.synchronize()
        assert same_bits(rows.get(), rows_a), "two calls from zeroed rows differ"
        assert same_bits(b["g_cur"].get(), g_cur) and same_bits(b["g_v_prev"].get(), g_vp)
        B.check()


@pytest.mark.parametrize("case", HD.LIF_CASES)
def test_lif_bwd_det_row_sums_exact_leg(case):
    """Dyadic data whose every term and partial sum is a float32 number (HD.lif_exact_inputs): the row sums array_equal the
    float64 reference, hard and soft reset, and a second call onto the same rows gives exactly twice -- one pixel's term lost,
    or added twice, anywhere in the reduction would show."""
    Bn, H, W, nrows = case
    npix = Bn * H * W
    nblk = HD.lif_bwd_grid(Bn, H, W, nrows)
    for hard in (True, False):
        B = Bufs()
        d = HD.lif_exact_inputs(case)
        b = lif_bufs(B, d, npix)
        r = HD.lif_bwd_ref64(d, hard, HD.ARCTAN, nblk)
        rows = B.new(np.zeros((nrows, ROW_LD), F32))
        for calls in (1, 2):
            assert lif_call(b, case, hard, HD.ARCTAN, rows) == 0
            torch.cuda.synchronize()
            got = rows.get()
            assert np.array_equal(got[:nblk, COL_LEAK:COL_LEAK + C].astype(F64), calls * r["rows_leak"]), (hard, calls)
            assert np.array_equal(got[:nblk, COL_THRESH:COL_THRESH + C].astype(F64), calls * r["rows_thresh"]), (hard, calls)
            tot = sum_rows(B, rows, nrows, ROW_LD)
            assert np.array_equal(tot[COL_LEAK:COL_LEAK + C].astype(F64), calls * r["g_leak"])
            assert np.array_equal(tot[COL_THRESH:COL_THRESH + C].astype(F64), calls * r["g_thresh"])
        assert np.array_equal(b["g_cur"].get().astype(F64), r["g_cur"]) and np.array_equal(b["g_v_prev"].get().astype(F64), r["g_v_prev"])
        B.check()


def test_lif_bwd_det_refusals():
    case = HD.LIF_CASES[0]
    Bn, H, W, nrows = case
    B = Bufs()
    b = lif_bufs(B, HD.lif_inputs(case), Bn * H * W)
    rows = B.new(np.full((nrows, ROW_LD), FILL, F32))
    assert lif_call(b, case, True, HD.ARCTAN, rows, row_ld=0) == EINVAL
    assert lif_call(b, case, True, HD.ARCTAN, rows, row_ld=-8) == EINVAL
    assert lif_call(b, case, True, HD.ARCTAN, rows, nrows=0) == EINVAL
    assert lif_call(b, (0, H, W, nrows), True, HD.ARCTAN, rows) == EINVAL
    torch.cuda.synchronize()
    assert np.all(rows.get() == FILL) and np.all(b["g_cur"].get() == FILL) and np.all(b["g_v_prev"].get() == FILL)
    B.check()


# ================================================================================================================ norm_input
def f64_buf(n, fill):
    t = torch.full((n + 16,), -724625.0, dtype=torch.float64, device=DEV)  # (guards of eight doubles either side)
    t[8:8 + n] = fill
    return t


def norm_call(name, x, n, out, ws, ws_doubles=None):
    if name == "evf_norm_nonzero":
        return call(name, x.ptr, n, out.ptr, ws[8:].data_ptr())
    return call(name, P(x), n, P(out), None if ws is None else ws[8:].data_ptr(), (ws.numel() - 16) if ws_doubles is None else ws_doubles)


@pytest.mark.parametrize("n", HD.NORM_N)
def test_norm_nonzero_det(n):
    """Voxel-like data, all zeros, exactly one non-zero entry: against float64 at the derived bound (NaN where the reference has
    NaN, +0.0 at every zero entry), two calls and a NaN-filled scratch the same bits, the default entry point inside the bound; a
    scratch one double short, or null, refused with the output untouched."""
    L = _lib.load()
    nws = int(L.evf_norm_nonzero_det_ws(n))
    assert nws == HD.norm_ws(n)
    for kind in ("voxel", "zeros", "one"):
        B = Bufs()
        x = HD.norm_inputs(n, kind)
        ref, scale = HD.norm_ref64(x)
        xb, out = B.new(x), B.new(np.full(n, FILL, F32))
        ws = f64_buf(nws, 1e300)
        assert norm_call("evf_norm_nonzero_det", xb, n, out, ws) == 0
        torch.cuda.synchronize()
        got = out.get()
        regime = f"norm_nonzero n={n} {kind}"
        within(regime, "out", got, ref, scale, HD.NORM_OPS)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.all(got[x == 0] == 0) and not np.signbit(got[x == 0]).any()
        if kind == "one":
            assert np.isnan(got).sum() == 1
        ws2 = f64_buf(nws, float("nan"))
        out.set(np.full(n, FILL, F32))
        assert norm_call("evf_norm_nonzero_det", xb, n, out, ws2) == 0
        torch.cuda.synchronize()
        assert same_bits(out.get(), got), "a NaN-filled scratch changes the result"
        assert norm_call("evf_norm_nonzero_det", xb, n, out, ws2) == 0
        torch.cuda.synchronize()
        assert same_bits(out.get(), got)
        for w in (ws, ws2):
            assert bool((w[:8] == -724625.0).all()) and bool((w[8 + nws:] == -724625.0).all()), "the scratch was overrun"
        ws3 = f64_buf(3, 0.0)
        out.set(np.full(n, FILL, F32))
        assert norm_call("evf_norm_nonzero", xb, n, out, ws3) == 0
        torch.cuda.synchronize()
        within(regime, "out (default entry)", out.get(), ref, scale, HD.NORM_OPS)
        # refusals
        out.set(np.full(n, FILL, F32))
        assert norm_call("evf_norm_nonzero_det", xb, n, out, ws, nws - 1) == EINVAL
        assert norm_call("evf_norm_nonzero_det", xb, n, out, None, nws) == EINVAL
        assert norm_call("evf_norm_nonzero_det", xb, 0, out, ws) == EINVAL
        torch.cuda.synchronize()
        assert np.all(out.get() == FILL)
        B.check()


# ================================================================================================================ graph replay
def test_graph_replay_gives_the_eager_bits():
    """The three twins captured once in a torch.cuda.graph and replayed twice on restored outputs: the eager bits."""
    L = _lib.load()
    B = Bufs()
    hcase = HD.HEAD_CASES[3]
    x, g = HD.head_inputs(hcase, "real")
    hx, hg = B.new(x), B.new(g)
    nsl, hn = L.evf_head_wgrad_det_slabs(hcase[0], hcase[2], hcase[3]), C * hcase[1] * 9
    slab = B.new(np.full((nsl, hn), FILL, F32))
    lcase = HD.LIF_CASES[1]
    npix = lcase[0] * lcase[1] * lcase[2]
    lb = lif_bufs(B, HD.lif_inputs(lcase), npix)
    rows = B.new(np.zeros((lcase[3], ROW_LD), F32))
    n = 1025
    nx, nout = B.new(HD.norm_inputs(n, "voxel")), B.new(np.full(n, FILL, F32))
    ws = f64_buf(HD.norm_ws(n), float("nan"))

    def restore():
        slab.set(np.full((nsl, hn), FILL, F32)), rows.set(np.zeros((lcase[3], ROW_LD), F32)), nout.set(np.full(n, FILL, F32))
        lb["g_cur"].set(np.full((npix, C), FILL, F32)), lb["g_v_prev"].set(np.full((npix, C), FILL, F32))

    def three_calls():
        assert head_call(hx, hg, hcase, slab, 0) == 0
        assert lif_call(lb, lcase, True, HD.ARCTAN, rows) == 0
        assert norm_call("evf_norm_nonzero_det", nx, n, nout, ws) == 0

    def snapshot():
        torch.cuda.synchronize()
        return {"slab": slab.get(), "rows": rows.get(), "g_cur": lb["g_cur"].get(), "g_v_prev": lb["g_v_prev"].get(), "norm": nout.get()}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        restore()
        three_calls()
        eager = snapshot()
        assert not np.any(eager["slab"] == FILL) and not np.any(eager["norm"] == FILL) and np.any(eager["rows"] != 0)
        restore()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            three_calls()
        for _ in range(2):
            restore()
            gr.replay()
            got = snapshot()
            for nm, ref in eager.items():
                assert same_bits(got[nm], ref), f"{nm} replayed differs from the eager calls"
    B.check()


# ================================================================================================================ routing
LIF_NEURON = {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}
PLIF_NEURON = {"leak_v": [-4.0, 0.1], "leak_pt": [-4.0, 0.1], "add_pt": [-2.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True,
               "learn_thresh": True, "hard_reset": True}
PAIRS = (("evf_head_wgrad", "evf_head_wgrad_det"), ("evf_lif_bwd", "evf_lif_bwd_det"), ("evf_norm_nonzero", "evf_norm_nonzero_det"))
BRACKET = [nm for p in PAIRS for nm in p]
DEFAULTS, DETS = {p[0] for p in PAIRS}, {p[1] for p in PAIRS}


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def loss_cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def model_cfg(neuron, num_bins, norm_input):
    return {"num_bins": num_bins, "base_num_channels": 32, "kernel_size": 3, "encoding": "voxel", "norm_input": norm_input,
            "mask_output": True, "activations": ["arctanspike", "arctanspike"], "spiking_neuron": dict(neuron)}


def voxel_passes(lists, num_bins, H, W):
    from event_flow_amd.dataloader.encodings import encode_event_list

    passes = [encode_event_list(ev, num_bins, (H, W), want=("cnt", "mask", "voxel", "pol")) for ev in lists]
    for d in passes:
        d["event_cnt"] = None  # (a voxel-encoded model must not need it)
    return passes


def alive(model):
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("thresh"):
                p.mul_(0.25)  # (an alive network: spikes in every layer)


def test_the_switch_routes_the_voxel_head_and_norm_input():
    """Profile brackets around one train_window of a voxel num_bins = 5 LIFFireNet with norm_input: with the switch on the three
    twins and none of the defaults, with it off the reverse; a backward follows the switch as it stood at its forward."""
    from event_flow_amd import synthetic, train
    from event_flow_amd.loss.flow import EventWarping
    from event_flow_amd.models.model import LIFFireNet

    Bn, n, H, W = 2, 400, 32, 40
    lists = [G(synthetic.event_list_batch(Bn, n, H, W, 9100 + k)) for k in range(2)]

    def seen(fn):
        _lib.profile_start(BRACKET)
        fn()
        return {k[0] for k, v in _lib.profile_stop().items() if v}

    before = _lib.deterministic()
    torch.manual_seed(0)
    model = LIFFireNet(model_cfg(LIF_NEURON, 5, True)).to(DEV)
    alive(model)
    model.train()
    assert model.compute_path[0] == "fused"
    opt = train.FlatAdam(model, lr=2e-4, clip=100.0, device_step=True)
    try:
        opt.zero_grad()
        lossf = EventWarping(loss_cfg(H, W), DEV)
        step = lambda: train.train_window(model, lossf, opt, voxel_passes(lists, 5, H, W))  # noqa: E731
        _lib.set_deterministic(True)
        assert seen(step) == DETS
        _lib.set_deterministic(False)
        assert seen(step) == DEFAULTS
        _lib.set_deterministic(True)
        assert seen(step) == DETS

        def forward_then_toggle(first, then):
            model.reset_states()
            d = voxel_passes(lists[:1], 5, H, W)[0]
            _lib.set_deterministic(first)
            out = model(d["event_voxel"], d["event_cnt"])
            _lib.set_deterministic(then)
            sum(f.sum() for f in out["flow"]).backward()
            model.reset_states()
            opt.zero_grad()

        assert seen(lambda: forward_then_toggle(True, False)) == DETS
        assert seen(lambda: forward_then_toggle(False, True)) == DEFAULTS
    finally:
        _lib.set_deterministic(before)
        opt.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from event_flow_amd import _lib, synthetic
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.models import engine
from event_flow_amd.models.model import LIFFireNet
assert not (engine.PARAM_ROWS and engine.TOP_FUSED)
names = ["evf_head_wgrad", "evf_lif_bwd", "evf_head_wgrad_det", "evf_lif_bwd_det"]
cfg = {"num_bins": 5, "base_num_channels": 32, "kernel_size": 3, "encoding": "voxel", "norm_input": False, "mask_output": True,
       "activations": ["arctanspike", "arctanspike"],
       "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.2, 0.02], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}
torch.manual_seed(0)
model = LIFFireNet(cfg).to("cuda:0")
model.train()
ev = torch.from_numpy(synthetic.event_list_batch(2, 400, 32, 40, 9100)).to("cuda:0")
_lib.set_deterministic(True)
d = encode_event_list(ev, 5, (32, 40), want=("voxel",))
_lib.profile_start(names)
out = model(d["event_voxel"], None)
try:
    sum(f.sum() for f in out["flow"]).backward()
    print("NO ERROR")
except _lib.EvflowError as e:
    print("RAISED EvflowError:", e)
seen = sorted(k[0] for k, v in _lib.profile_stop().items() if v)
print("SEEN", seen)
"""


@pytest.mark.parametrize("var", ("EVF_PARAM_ROWS", "EVF_TOP_FUSED"))
def test_a_route_that_would_add_with_atomics_raises(var):
    """EVF_PARAM_ROWS=0 (no per-block rows: every per-channel sum an atomic) and EVF_TOP_FUSED=0 (evf_pred_bwd), read at import, so
    in a fresh child process: the deterministic voxel backward raises EvflowError naming the switch and launches neither the twins
    nor the atomics."""
    env = dict(os.environ, **{var: "0"})
    env.pop("EVF_DETERMINISTIC", None)
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "RAISED EvflowError" in out.stdout and var in out.stdout, out.stdout
    assert "SEEN []" in out.stdout, out.stdout


def test_a_fused_alif_network_is_refused(det_on):
    """A fused ALIFFireNet's prediction-head backward is evf_pred_bwd (66 float atomics per block): with the switch on the
    backward raises EvflowError naming it instead of running it; with the switch off the same window runs."""
    from event_flow_amd import synthetic
    from event_flow_amd.dataloader.encodings import encode_event_list
    from event_flow_amd.models.model import ALIFFireNet

    neuron = {"leak_v": [-4.0, 0.1], "leak_t": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
              "learn_thresh": True, "hard_reset": True}
    cfg = dict(model_cfg(neuron, 2, False), encoding="cnt")
    torch.manual_seed(0)
    m = ALIFFireNet(cfg).to(DEV)
    m.train()
    assert m.compute_path[0] == "fused"
    d = encode_event_list(G(synthetic.event_list_batch(2, 400, 32, 40, 9400)), 2, (32, 40), want=("cnt",))
    _lib.profile_start(["evf_pred_bwd"])
    out = m(None, d["event_cnt"])
    with pytest.raises(_lib.EvflowError, match="evf_pred_bwd"):
        sum(f.sum() for f in out["flow"]).backward()
    assert not any(v for v in _lib.profile_stop().values())
    m.reset_states()
    _lib.set_deterministic(False)
    _lib.profile_start(["evf_pred_bwd"])
    out = m(None, d["event_cnt"])
    sum(f.sum() for f in out["flow"]).backward()
    assert any(v for v in _lib.profile_stop().values())


LM_CHILD = r"""
import copy, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from event_flow_amd import _lib, synthetic
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.loss.flow import EventWarping
from event_flow_amd.models import engine
from event_flow_amd.models.model import PLIFFireNet
from event_flow_amd.train import FlatAdam, train_window
assert not engine.FUSED_TAIL and engine.PLIF_LAYER_MAJOR
H, W = 32, 40
cfg = {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "voxel", "norm_input": True, "mask_output": True,
       "activations": ["arctanspike", "arctanspike"],
       "spiking_neuron": {"leak_v": [-4.0, 0.1], "leak_pt": [-4.0, 0.1], "add_pt": [-2.0, 0.1], "thresh": [0.2, 0.02], "learn_leak": True,
                          "learn_thresh": True, "hard_reset": True}}
lists = [[torch.from_numpy(synthetic.event_list_batch(2, 400, H, W, 9500 + 10 * w + k)).to("cuda:0") for k in range(3)] for w in range(2)]
torch.manual_seed(0)
sd0 = copy.deepcopy(PLIFFireNet(cfg).to("cuda:0").state_dict())
_lib.set_deterministic(True)
names = ["evf_sum_rows", "evf_plif_bwd_wgrad_window", "evf_plif_bwd_wgrad_window_top", "evf_grads_finalize", "evf_reduce_slabs"]
res = []
for run in range(2):
    m = PLIFFireNet(cfg).to("cuda:0")
    m.load_state_dict(sd0)
    m.train()
    opt = FlatAdam(m, lr=2e-4, clip=100.0, device_step=True)
    opt.zero_grad()
    lossf = EventWarping({"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
                          "model": {"mask_output": True}}, "cuda:0")
    _lib.profile_start(names)
    for w in range(2):
        passes = [encode_event_list(ev, 2, (H, W), want=("cnt", "mask", "voxel", "pol")) for ev in lists[w]]
        train_window(m, lossf, opt, passes)
    seen = sorted(k for k, v in _lib.profile_stop().items() if v)
    res.append((opt.flat_param.clone(), opt.m.clone(), opt.v.clone()))
    assert float(opt.m.abs().max()) > 0
    opt.close()
print("SEEN", seen)
print("EQUAL", all(torch.equal(a, b) for a, b in zip(*res)))
"""


def test_the_layer_major_plif_window_gets_the_fixed_order_tail():
    """EVF_FUSED_TAIL=0 in a fresh child process, a PLIF voxel num_bins = 2 FireNet with norm_input under train_window: its
    backward is the layer-major window route (evf_plif_bwd_wgrad_window[_top]), which never enters _backward_pass.  With the
    switch on every evf_sum_rows of the step-by-step tail is the non-accumulating, single-writer form (never the float-atomic
    accumulating one), evf_grads_finalize and evf_reduce_slabs do not run, and two runs of two windows end torch.equal."""
    env = dict(os.environ, EVF_FUSED_TAIL="0")
    env.pop("EVF_DETERMINISTIC", None)
    env.pop("EVF_PLIF_LAYER_MAJOR", None)
    out = subprocess.run([sys.executable, "-c", LM_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = out.stdout.split("SEEN", 1)[1].splitlines()[0]
    assert "evf_plif_bwd_wgrad_window" in seen, out.stdout  # (the layer-major route was what ran)
    assert "('evf_sum_rows', 'set')" in seen and "('evf_sum_rows', 'acc')" not in seen, out.stdout
    assert "evf_grads_finalize" not in seen and "'evf_reduce_slabs'" not in seen, out.stdout
    assert "EQUAL True" in out.stdout, out.stdout


def test_the_step_by_step_tail_adds_in_a_fixed_order(det_on):
    """Gradients handed to autograd (no FlatAdam, so no evf_grads_finalize): a voxel num_bins = 5 LIFFireNet window with norm_input
    through the real loss, twice from one state_dict -- every parameter gradient torch.equal, the head weight's non-zero in all
    five input planes, and the twins are what ran."""
    from event_flow_amd import synthetic
    from event_flow_amd.loss.flow import EventWarping
    from event_flow_amd.models.model import LIFFireNet

    Bn, n, H, W = 2, 400, 32, 40
    lists = [G(synthetic.event_list_batch(Bn, n, H, W, 9300 + k)) for k in range(3)]
    torch.manual_seed(5)
    first = LIFFireNet(model_cfg(LIF_NEURON, 5, True)).to(DEV)
    alive(first)
    sd0 = copy.deepcopy(first.state_dict())
    grads = []
    for run in range(2):
        m = LIFFireNet(model_cfg(LIF_NEURON, 5, True)).to(DEV)
        m.load_state_dict(sd0)
        m.train()
        lossf = EventWarping(loss_cfg(H, W), DEV)
        _lib.profile_start(BRACKET)
        for d in voxel_passes(lists, 5, H, W):
            out = m(d["event_voxel"], d["event_cnt"])
            lossf.event_flow_association(out["flow"], d["event_list"], d["event_list_pol_mask"], d["event_mask"])
        lossf().backward()
        assert {k[0] for k, v in _lib.profile_stop().items() if v} == DETS
        assert all(p.grad is not None for p in m.parameters())
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    gw = grads[0]["head.ff.weight"]
    assert tuple(gw.shape) == (32, 5, 3, 3) and bool((gw.abs().amax(dim=(0, 2, 3)) > 0).all())
    assert all(float(g.abs().max()) > 0 for g in grads[0].values()), [k for k, g in grads[0].items() if float(g.abs().max()) == 0]


# ================================================================================================================ whole steps
def _steps(cls, neuron, num_bins, norm_input, runs):
    """tests/test_gpu_deterministic.py's harness for a voxel-encoded model: every run starts from the same state_dict and trains
    three windows (2 x 32 x 40, three passes of 400 events) through the real EventWarping with FlatAdam, static states and a
    device-side step counter; "graph": the third window is captured into a hipGraph and replayed instead of launched.
    -> per run (parameters, Adam m, Adam v, recurrent states, the head weight's gradient [32,Cin,3,3] of the first two windows)."""
    from event_flow_amd import synthetic
    from event_flow_amd.loss import flow as hloss
    from event_flow_amd.train import FlatAdam, train_window, window_apply, window_backward

    Bn, n, H, W, NP = 2, 400, 32, 40, 3
    pool = [[G(synthetic.event_list_batch(Bn, n, H, W, 7300 + 100 * w + k)) for k in range(NP)] for w in range(3)]
    assert all(float((ev[:, :, 0] % 1).abs().max()) > 0 for w in pool for ev in w)  # fractional timestamps: real-valued voxels
    torch.manual_seed(3)
    first = cls(model_cfg(neuron, num_bins, norm_input)).to(DEV)
    alive(first)
    sd0 = copy.deepcopy(first.state_dict())

    head_grads = []

    def step(model, lossf, opt, lists, grab=False):
        if not grab:
            return train_window(model, lossf, opt, voxel_passes(lists, num_bins, H, W))
        loss = window_backward(model, lossf, opt, voxel_passes(lists, num_bins, H, W))  # train_window's two halves, the gradient
        head_grads.append(model.head.ff.weight.grad.detach().clone())                  # read in between
        return window_apply(model, lossf, opt, loss, None)

    out = []
    for kind in runs:
        m = cls(model_cfg(neuron, num_bins, norm_input)).to(DEV)
        m.load_state_dict(sd0)
        m.train()
        assert m.compute_path[0] == "fused"
        opt = FlatAdam(m, lr=2e-4, clip=100.0, device_step=True)
        opt.zero_grad()
        start = opt.flat_param.clone()
        m.use_static_states(True)
        lossf = hloss.EventWarping(loss_cfg(H, W), DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            losses = [step(m, lossf, opt, pool[w], grab=True) for w in range(2)]
            torch.cuda.synchronize()
            if kind == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    step(m, lossf, opt, pool[2])
                g.replay()
            else:
                losses.append(step(m, lossf, opt, pool[2]))
            torch.cuda.synchronize()
        assert float(opt.norm_ws[1]) == 3.0 and all(np.isfinite(float(x)) for x in losses)
        assert float((opt.flat_param - start).abs().max()) > 0  # (it trained)
        out.append((opt.flat_param.clone(), opt.m.clone(), opt.v.clone(), [s.clone() for s in m.states], head_grads[-2:]))
        head_grads = []
        opt.close()
    return out


def _same(a, b):
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ("LIF voxel 5 norm", "PLIF voxel 5", "LIF voxel 2 norm"))
def test_voxel_training_steps_repeat_bit_for_bit_through_the_real_loss(det_on, name):
    """Two independent eager runs of three windows from one state_dict, and the third window replayed from a captured hipGraph:
    parameters, both Adam moments and all recurrent states torch.equal.  num_bins = 2 is the real-valued two-channel input of the
    slab kernels (evf_head_lif_bwd_wgrad / the window kernels).  The head weight's gradient reached every input plane."""
    from event_flow_amd.models.model import LIFFireNet, PLIFFireNet

    cls, neuron, nb, norm = {"LIF voxel 5 norm": (LIFFireNet, LIF_NEURON, 5, True), "PLIF voxel 5": (PLIFFireNet, PLIF_NEURON, 5, False),
                             "LIF voxel 2 norm": (LIFFireNet, LIF_NEURON, 2, True)}[name]
    eager1, eager2, graph = _steps(cls, neuron, nb, norm, ["eager", "eager", "graph"])
    _same(eager1, eager2)
    _same(eager1, graph)
    for run in (eager1, eager2, graph):
        for w, gw in enumerate(run[4]):
            assert tuple(gw.shape) == (32, nb, 3, 3) and torch.equal(gw, eager1[4][w])
            assert bool((gw.abs().amax(dim=(0, 2, 3)) > 0).all()), "an input plane of the head weight received no gradient"
