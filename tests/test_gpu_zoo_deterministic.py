"""Deterministic mode for the non-spiking zoo: evf_chan_reduce_det (norm statistics and every bias gradient),
evf_leaky_bwd_det (g_leak of the leaky cells) and evf_conv2d_wgrad_det (generic-kernel-size weight gradients) through the C ABI
against the float64 references of tests/zoo_det_ref.py at the bounds stated there, bit for bit from call to call, from a
NaN-filled scratch and from a captured hipGraph; the host routing behind EVF_DETERMINISTIC / set_deterministic; and whole
training steps of FireNet, LeakyFireNet, a batch-norm EV-FlowNet and a 5x5 LIF-FireNet repeated bit for bit.

EVF_DET_ZOO_REPORT=<file>: the largest observed error of every regime as a fraction of its bound is written there."""

import copy
import os

import numpy as np
import pytest
import torch

import conv_ref as CR
import neuron_gen_ref as R
import zoo_det_ref as Z
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32, F64 = np.float32, np.float64
FILL = 7.0  # initial contents of outputs that a kernel must overwrite (or must leave alone)

REPORT = {}  # regime -> {output: fraction of its bound}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("EVF_DET_ZOO_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write(f"bounds in units of 2^-24 * sum |terms|: chan_reduce ops (0 / 2 / 3) + chain; g_leak K_LEAKY {R.K_LEAKY:g} + chain; "
                    f"bias and weight gradient K_SUM {CR.K_SUM:g}\n")
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


def note(regime, name, frac):
    r = REPORT.setdefault(regime, {})
    r[name] = max(r.get(name, 0.0), float(frac))


def call(name, *args):
    return _lib.raw(name, *args)


def P(b):
    return None if b is None else b.ptr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def within(regime, name, got, ref, scale, k, extra=0.0):
    """|got - ref| <= k * 2^-24 * (scale + extra) everywhere; prints and records the fraction of the bound that was used."""
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64)).reshape(-1)
    bound = k * Z.U * (np.asarray(scale, F64) + extra).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(frac)) if frac.size else 0
    worst = float(frac[i]) if frac.size else 0.0
    print(f"  {regime} {name}: {worst:.3f} of the bound")
    note(regime, name, worst)
    assert worst <= 1.0, f"{regime} {name}: error {err[i]:.4g} > bound {bound[i]:.4g} at {i}"


def scratch(B, n, fill=None):
    rng = np.random.default_rng(n)
    return B.new(rng.normal(0, 1e3, n).astype(F32) if fill is None else np.full(n, fill, F32))  # (need not be zero on entry)


# ============================================================================================================== chan_reduce
def chan_call(d, mode, out, acc, ws, ws_floats=None):
    has = mode == 2
    return call("evf_chan_reduce_det", d["x"].ptr, d["ld"], d["y"].ptr if has else None, d["ld"] if has else 0,
                d["center"].ptr if mode else None, d["scale"].ptr if has else None, mode, d["G"], d["npg"], d["C"], out.ptr, acc,
                P(ws), (ws.t.numel() if ws is not None else d["n_ws"]) if ws_floats is None else ws_floats)


@pytest.mark.parametrize("npg", Z.CHAN_NPG)
@pytest.mark.parametrize("C", Z.CHAN_C)
def test_chan_reduce_det(C, npg):
    """The three modes, one and three groups, pixel strides C and C + 4, accumulate 0 and 1 onto a random output: against float64
    within (ops + chain) * 2^-24 * sum |terms|; a second call and a call on a NaN-filled scratch give the same bits; a scratch
    one float short, or null, is refused and the output untouched."""
    lib = _lib.load()
    for G in Z.CHAN_G:
        g = Z.chan_geometry(G, npg, C)
        n_ws = int(lib.evf_chan_reduce_det_ws(G, npg, C))
        assert n_ws >= G * g["rows"] * g["cols"]
        for pad in (0, 4):
            regime = f"chan_reduce G={G} npg={npg} C={C} ld={C + pad} ({g['bpg']} blocks per group, chain {g['chain']})"
            x, y, center, scale, init = Z.chan_inputs(G, npg, C, pad)
            B = Bufs()
            d = {"x": B.new(x), "y": B.new(y), "center": B.new(center), "scale": B.new(scale), "ld": C + pad, "G": G, "npg": npg,
                 "C": C, "n_ws": n_ws}
            ws, nan = scratch(B, n_ws), scratch(B, n_ws, np.nan)
            for mode in (0, 1, 2):
                ref, sab = Z.chan_ref64(x, y, center, scale, mode, G, npg, C)
                k = Z.CHAN_OPS[mode] + g["chain"]
                for acc in (0, 1):
                    outs = [B.new(init) for _ in range(3)]
                    assert chan_call(d, mode, outs[0], acc, ws) == 0
                    assert chan_call(d, mode, outs[1], acc, ws) == 0  # (the scratch as the first call left it)
                    assert chan_call(d, mode, outs[2], acc, nan) == 0
                    got = outs[0].get()
                    within(regime, f"mode {mode}" + (" accumulated" if acc else ""), got, ref + (init if acc else 0), sab, k,
                           extra=np.abs(init.astype(F64)) if acc else 0.0)
                    assert same_bits(got, outs[1].get()), f"{regime}: mode {mode} differs between two calls"
                    assert same_bits(got, outs[2].get()), f"{regime}: mode {mode} depends on the contents of the scratch"
                untouched = B.new(init)
                assert chan_call(d, mode, untouched, 0, ws, ws_floats=n_ws - 1) == EINVAL
                assert chan_call(d, mode, untouched, 0, None) == EINVAL
                torch.cuda.synchronize()
                assert same_bits(untouched.get(), init), f"{regime}: a refused call wrote the output"
            B.check()


def test_chan_reduce_det_refuses_what_the_default_refuses():
    B = Bufs()
    x, out, ws = B.new(np.ones((8, 8), F32)), B.new(np.full(8, FILL, F32)), B.new(np.zeros(1 << 12, F32))

    def red(x_=x.ptr, ldx=8, y=None, ldy=0, mode=0, G=1, npg=8, C=8, out_=out.ptr):
        return call("evf_chan_reduce_det", x_, ldx, y, ldy, None, None, mode, G, npg, C, out_, 0, ws.ptr, ws.t.numel())

    assert red(x_=None) == EINVAL and red(out_=None) == EINVAL and red(G=0) == EINVAL and red(npg=0) == EINVAL and red(C=0) == EINVAL
    assert red(ldx=7) == EINVAL and red(mode=3) == EINVAL and red(mode=-1) == EINVAL
    assert red(mode=2) == EINVAL and red(mode=2, y=x.ptr, ldy=7) == EINVAL
    torch.cuda.synchronize()
    assert np.all(out.get() == FILL)
    assert red() == 0
    assert np.all(out.get() == 8.0)
    B.check()


@pytest.mark.parametrize("Cout", Z.BIAS_COUT)
def test_bias_gradient_at_the_project_bar(Cout):
    """The bias gradient of deterministic mode = evf_chan_reduce_det, mode 0, one group over g_y [M][ldg], ldg > Cout: against
    g_y.sum in float64 at K_SUM * 2^-24 * sum |g|, the bar test_dense_weight_gradient holds the default's bias gradient to."""
    gy, init = Z.bias_inputs(Cout)
    B = Bufs()
    n_ws = int(_lib.load().evf_chan_reduce_det_ws(1, Z.BIAS_M, Cout))
    d = {"x": B.new(gy), "ld": gy.shape[1], "G": 1, "npg": Z.BIAS_M, "C": Cout, "n_ws": n_ws}
    ws = scratch(B, n_ws)
    ref, sab = Z.chan_ref64(gy, None, None, None, 0, 1, Z.BIAS_M, Cout)
    for acc in (0, 1):
        out = B.new(init)
        assert chan_call(d, 0, out, acc, ws) == 0
        within(f"bias gradient Cout={Cout}", "accumulated" if acc else "overwritten", out.get(), ref[0] + (init if acc else 0), sab[0],
               CR.K_SUM, extra=np.abs(init.astype(F64)) if acc else 0.0)
    B.check()


# ==================================================================================================================== leaky
PREV_MODES = ("present", "absent", "no_g_prev")


def leaky_bwd(entry, b, act_id, npix, C, g_cur, g_prev, g_leak, ws=None, ws_floats=None):
    tail = () if entry == "evf_leaky_bwd" else (P(ws), (ws.t.numel() if ws is not None else 1 << 20) if ws_floats is None else ws_floats)
    return call(entry, P(b["g_out"]), P(b["g_state"]), b["mix"].ptr, P(b["prev"]), b["leak"].ptr, act_id, npix, C, g_cur.ptr, P(g_prev),
                P(g_leak), *tail)


@pytest.mark.parametrize("C,npix", R.SMALL_SHAPES + R.BLOCK_SHAPES)
def test_leaky_bwd_det(C, npix):
    """The shuffle arm, shuffle + turns, Q > 64, a Q that is no power of two, the 1024-block cap with several trips; activation
    none / relu / tanh, previous state present / absent / present without a gradient, g_out only / g_state only / both (the full
    cross on the small shapes, three combinations that cover every value on the large ones).  g_cur / g_prev: evf_leaky_bwd's
    bits; g_leak against float64 at the bound of the default entry's test with this kernel's chain; repeat, NaN scratch,
    refusals; afterwards one default call still gives its usual result (the replica array was left alone)."""
    from test_gpu_neuron_gen import leaky_chain  # (the chain of the default entry, as its own test counts it)

    lib = _lib.load()
    g = Z.leaky_geometry(C, npix)
    regime = f"leaky C={C} npix={npix} (Q={g['Q']}, {g['nblk']} blocks x {g['bs']}, {g['trips']} trips, {g['arm']}, chain {g['chain']})"
    d = Z.leaky_inputs(C, npix)
    n = (npix, C)
    n_ws = int(lib.evf_leaky_bwd_det_ws(npix, C))
    assert n_ws >= g["rows"] * g["cols"]
    combos = [(a, p, u) for a in Z.LEAKY_ACTS for p in PREV_MODES for u in Z.LEAKY_UPSTREAM]
    if npix > 1000:
        combos = [(Z.LEAKY_ACTS[i], PREV_MODES[i], Z.LEAKY_UPSTREAM[i]) for i in range(3)]
    fill = np.full(n, FILL, F32)
    init = d["init"]
    for (act_id, act), pmode, up in combos:
        B = Bufs()
        has_prev = pmode != "absent"
        cb, lb = B.new(d["cur"]), B.new(d["leak"])
        pb = B.new(d["prev"]) if has_prev else None
        mix = B.new(fill)
        assert call("evf_leaky_fwd", cb.ptr, P(pb), None, lb.ptr, act_id, npix, C, mix.ptr, None) == 0
        go = d["g_out"] if up in ("both", "out") else None
        gs = d["g_state"] if up in ("both", "state") else None
        ref = Z.leaky_reference(mix.get(), d["prev"] if has_prev else None, d["leak"], act, go, gs)
        b = {"g_out": B.new(go) if go is not None else None, "g_state": B.new(gs) if gs is not None else None, "mix": mix, "prev": pb,
             "leak": lb}
        ws, nan = scratch(B, n_ws), scratch(B, n_ws, np.nan)

        def outputs():
            return B.new(fill), (B.new(fill) if pmode == "present" else None), B.new(init)

        first, again, fromnan, default = outputs(), outputs(), outputs(), outputs()
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, *first, ws) == 0
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, *again, ws) == 0
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, *fromnan, nan) == 0
        within(regime, "g_cur", first[0].get(), ref["g_cur"], ref["s_g_cur"], R.K_LEAKY)
        within(regime, "g_leak", first[2].get(), init.astype(F64) + ref["g_leak"], ref["s_g_leak"], R.K_LEAKY + g["chain"],
               extra=np.abs(init.astype(F64)))
        for other, what in ((again, "differs between two calls"), (fromnan, "depends on the contents of the scratch")):
            for i, nm in enumerate(("g_cur", "g_prev", "g_leak")):
                if first[i] is not None:
                    assert same_bits(first[i].get(), other[i].get()), f"{regime}: {nm} {what}"
        # a null g_leak: nothing summed, the element-wise outputs all the same
        nol = B.new(fill)
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, nol, None, None, ws) == 0
        assert same_bits(nol.get(), first[0].get())
        untouched = outputs()
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, *untouched, ws, ws_floats=n_ws - 1) == EINVAL
        assert leaky_bwd("evf_leaky_bwd_det", b, act_id, npix, C, *untouched, None, ws_floats=n_ws) == EINVAL
        torch.cuda.synchronize()
        assert np.all(untouched[0].get() == FILL) and same_bits(untouched[2].get(), init), f"{regime}: a refused call wrote an output"
        # the default entry afterwards: the same element-wise bits, its usual g_leak
        assert leaky_bwd("evf_leaky_bwd", b, act_id, npix, C, *default) == 0
        assert same_bits(first[0].get(), default[0].get()), f"{regime}: g_cur differs from evf_leaky_bwd's"
        if first[1] is not None:
            within(regime, "g_prev", first[1].get(), ref["g_prev"], ref["s_g_prev"], R.K_LEAKY)
            assert same_bits(first[1].get(), default[1].get()), f"{regime}: g_prev differs from evf_leaky_bwd's"
        within(regime, "g_leak of the default entry afterwards", default[2].get(), init.astype(F64) + ref["g_leak"], ref["s_g_leak"],
               R.K_LEAKY + leaky_chain(C, npix) + 1, extra=np.abs(init.astype(F64)))
        B.check()


def test_leaky_bwd_det_refuses_what_the_default_refuses():
    B = Bufs()
    x, lk, ws = B.new(np.zeros((3, 8), F32)), B.new(np.zeros(8, F32)), B.new(np.zeros(1 << 12, F32))
    b = {"g_out": x, "g_state": None, "mix": x, "prev": None, "leak": lk}
    out = B.new(np.full((3, 8), FILL, F32))
    assert leaky_bwd("evf_leaky_bwd_det", dict(b, g_out=None), 0, 3, 8, out, None, None, ws) == EINVAL
    assert leaky_bwd("evf_leaky_bwd_det", b, 4, 3, 8, out, None, None, ws) == EINVAL
    assert leaky_bwd("evf_leaky_bwd_det", b, 0, 4, 6, out, None, None, ws) == EINVAL
    assert leaky_bwd("evf_leaky_bwd_det", b, 0, 0, 8, out, None, None, ws) == EINVAL
    torch.cuda.synchronize()
    assert np.all(out.get() == FILL)
    B.check()


# ==================================================================================================================== wgrad
def wgrad_call(x, ldx, gy, g_w, shape, ws, ws_floats=None, cin_total=None, cin_off=0, accumulate=2, g_bias=None):
    Bn, H, W, Cin, Cout, k, s = shape
    return call("evf_conv2d_wgrad_det", x.ptr, ldx, gy.ptr, Cout, g_w.ptr, P(g_bias), Bn, H, W, Cin, Cout, k, s,
                Cin if cin_total is None else cin_total, cin_off, accumulate, P(ws),
                (ws.t.numel() if ws is not None else 1 << 24) if ws_floats is None else ws_floats)


def check_wgrad_det(shape, cin_total=None, cin_off=0):
    """-> nothing; one shape against conv_wgrad64 at K_SUM, then repeat / NaN scratch / refusals."""
    Bn, H, W, Cin, Cout, k, s = shape
    lib = _lib.load()
    g = Z.wgrad_det_geometry(*shape)
    regime = f"wgrad {shape}" + (f" into channels {cin_off}.. of {cin_total}" if cin_total else "") + \
        (f" ({g['ksplit']} splits x {g['stages']} stages, CT {g['CT']} NT {g['NT']})" if k != 3 else " (forwarded)")
    n_ws = int(lib.evf_conv2d_wgrad_det_ws(*shape))
    assert n_ws >= (g["rows"] * g["cols"] if k != 3 else 1)
    x, gy = Z.wgrad_inputs(shape)
    ct = Cin if cin_total is None else cin_total
    acc = 1 if cin_total else 0
    rng = np.random.default_rng(Cin)
    init = rng.normal(0, 3, (Cout, ct, k, k)).astype(F32) if acc else np.full((Cout, ct, k, k), FILL, F32)
    ref, sab = init.astype(F64) * acc, np.abs(init.astype(F64)) * acc
    ref[:, cin_off:cin_off + Cin] += CR.conv_wgrad64(x, gy, k, s)
    sab[:, cin_off:cin_off + Cin] += CR.conv_wgrad64(np.abs(x), np.abs(gy), k, s)
    B = Bufs()
    xb, gb = B.new(x), B.new(gy)
    ws, nan = scratch(B, n_ws), scratch(B, n_ws, np.nan)
    outs = [B.new(init) for _ in range(3)]
    kw = {"cin_total": cin_total, "cin_off": cin_off, "accumulate": 2 | acc}  # (2: x is not spike-valued)
    assert wgrad_call(xb, Cin, gb, outs[0], shape, ws, **kw) == 0
    assert wgrad_call(xb, Cin, gb, outs[1], shape, ws, **kw) == 0
    assert wgrad_call(xb, Cin, gb, outs[2], shape, nan, **kw) == 0
    got = outs[0].get()
    within(regime, "g_w", got, ref, sab, CR.K_SUM)
    assert same_bits(got, outs[1].get()), f"{regime}: differs between two calls"
    assert same_bits(got, outs[2].get()), f"{regime}: depends on the contents of the scratch"
    untouched, bias = B.new(init), B.new(np.full(Cout, FILL, F32))
    assert wgrad_call(xb, Cin, gb, untouched, shape, ws, ws_floats=n_ws - 1, **kw) == EINVAL
    assert wgrad_call(xb, Cin, gb, untouched, shape, None, ws_floats=n_ws, **kw) == EINVAL
    assert wgrad_call(xb, Cin, gb, untouched, shape, ws, g_bias=bias, **kw) == EINVAL  # (the bias is evf_chan_reduce_det's)
    torch.cuda.synchronize()
    assert same_bits(untouched.get(), init) and np.all(bias.get() == FILL), f"{regime}: a refused call wrote an output"
    B.check()


@pytest.mark.parametrize("shape", Z.WGRAD_SHAPES)
def test_wgrad_det_generic_kernel_sizes(shape):
    """5x5 with K splits and unaligned channel counts, 5x5 stride 2 on 2 x 2 tiles, 7x7, and the 1x1 with more than four outputs."""
    assert _lib.load().evf_conv2d_wgrad_ws(*shape) == 0  # (no scratch: shapes the default entry serves with atomics)
    check_wgrad_det(shape)


def test_wgrad_det_into_a_channel_range_accumulating():
    shape, cin_total, cin_off = Z.WGRAD_OFFSET_CASE
    check_wgrad_det(shape, cin_total, cin_off)


def test_wgrad_det_forwards_the_3x3():
    check_wgrad_det(Z.WGRAD_FORWARD_CASE)


# ============================================================================================================= graph replay
def test_det_calls_replay_from_a_graph_as_they_run_eagerly():
    """One evf_chan_reduce_det, one evf_leaky_bwd_det and one evf_conv2d_wgrad_det call: captured on a side stream and replayed
    twice from restored outputs, against the same three calls launched eagerly -- bit for bit."""
    lib = _lib.load()
    B = Bufs()
    G, npg, C = 3, 700, 96
    x, y, center, scale, init = Z.chan_inputs(G, npg, C, 4)
    cd = {"x": B.new(x), "y": B.new(y), "center": B.new(center), "scale": B.new(scale), "ld": C + 4, "G": G, "npg": npg, "C": C}
    cws = scratch(B, int(lib.evf_chan_reduce_det_ws(G, npg, C)))
    cout = B.new(init)
    LC, lnpix = 24, 45000
    d = Z.leaky_inputs(LC, lnpix)
    mix = B.new(Z.leaky_mix32(d["cur"], d["prev"], d["leak"]))
    lb = {"g_out": B.new(d["g_out"]), "g_state": B.new(d["g_state"]), "mix": mix, "prev": B.new(d["prev"]), "leak": B.new(d["leak"])}
    lws = scratch(B, int(lib.evf_leaky_bwd_det_ws(lnpix, LC)))
    fill = np.full((lnpix, LC), FILL, F32)
    louts = (B.new(fill), B.new(fill), B.new(d["init"]))
    shape = Z.WGRAD_SHAPES[0]
    wx, wgy = Z.wgrad_inputs(shape)
    wxb, wgb = B.new(wx), B.new(wgy)
    wws = scratch(B, int(lib.evf_conv2d_wgrad_det_ws(*shape)))
    winit = np.full((shape[4], shape[3], shape[5], shape[5]), FILL, F32)
    wout = B.new(winit)

    def restore():
        cout.set(init), louts[0].set(fill), louts[1].set(fill), louts[2].set(d["init"]), wout.set(winit)

    def three_calls():
        assert chan_call(cd, 2, cout, 1, cws) == 0
        assert leaky_bwd("evf_leaky_bwd_det", lb, 1, lnpix, LC, *louts, lws) == 0
        assert wgrad_call(wxb, shape[3], wgb, wout, shape, wws) == 0

    def snapshot():
        torch.cuda.synchronize()
        return {"chan": cout.get(), "g_cur": louts[0].get(), "g_prev": louts[1].get(), "g_leak": louts[2].get(), "g_w": wout.get()}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        restore()
        three_calls()
        eager = snapshot()
        assert not same_bits(eager["chan"], init) and not same_bits(eager["g_leak"], d["init"]) and not np.any(eager["g_w"] == FILL)
        restore()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            three_calls()
        for _ in range(2):
            restore()
            g.replay()
            got = snapshot()
            for nm, ref in eager.items():
                assert same_bits(got[nm], ref), f"{nm} replayed differs from the eager calls"
    B.check()


# ================================================================================================================== routing
PAIRS = (("evf_chan_reduce", "evf_chan_reduce_det"), ("evf_leaky_bwd", "evf_leaky_bwd_det"), ("evf_conv2d_wgrad", "evf_conv2d_wgrad_det"))
BRACKET = [n for p in PAIRS for n in p]
DETS = {p[1] for p in PAIRS}
LOSS_CFG = {"loader": {"resolution": [64, 64]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}
LEAKY = {"leak": [-1.0, 0.5], "learn_leak": True}
LIF = {"leak": [-4.0, 0.1], "thresh": [0.25, 0.05], "learn_leak": True, "learn_thresh": True, "hard_reset": True}


def windows(nwin=2, B=2, n=3000, H=64, W=64):
    from event_flow_amd import synthetic
    from event_flow_amd.train import encode_passes

    return [encode_passes([torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 777 + 13 * w)).to(DEV)], 2, (H, W))
            for w in range(nwin)]


def make_model(name):
    """FireNet / LeakyFireNet (base 32), LIFFireNet with 5x5 kernels (base 32), an EV-FlowNet whose layers carry batch norm (base 8:
    the model class fixes norm = None, so its UNet is rebuilt with the same arguments and norm = "BN")."""
    from event_flow_amd.models import model as M
    from event_flow_amd.models import unet

    cfg = {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
           "activations": ["relu", None], "spiking_neuron": None}
    if name == "LeakyFireNet":
        cfg["spiking_neuron"] = dict(LEAKY)
    elif name == "LIFFireNet k5":
        cfg.update(kernel_size=5, activations=["arctanspike", "arctanspike"], spiking_neuron=dict(LIF))
    elif name == "EVFlowNet BN":
        cfg["base_num_channels"] = 8
        model = M.EVFlowNet(cfg)
        kw = {"num_bins": 2, "base_num_channels": 8, "kernel_size": 3, "activations": ["relu", None], "num_encoders": 4,
              "num_residual_blocks": 2, "num_output_channels": 2, "skip_type": "concat", "norm": "BN", "use_upsample_conv": True,
              "channel_multiplier": 2, "final_activation": "tanh"}
        model.multires_unet = unet.MultiResUNet(kw)
        assert any(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules())
        return model.to(DEV)
    model = getattr(M, name.split()[0])(cfg).to(DEV)
    if name == "LIFFireNet k5":
        assert not model._fused()
    return model


def test_the_switch_routes_the_zoo():
    """Profile brackets around one train_window of a LeakyFireNet and of a batch-norm EV-FlowNet (2 x 64 x 64, 3000 events): with the
    switch on the deterministic entry points and none of the default ones, with it off the reverse; a Function follows the switch
    as it stood in its forward."""
    from event_flow_amd import train
    from event_flow_amd.loss.flow import EventWarping

    win = windows(1)[0]

    def seen(fn):
        _lib.profile_start(BRACKET)
        fn()
        return {k[0] for k, v in _lib.profile_stop().items() if v}

    before = _lib.deterministic()
    opts = []
    try:
        # (LeakyFireNet has no norm layer: evf_chan_reduce_det is its bias gradients, which the default mode sums inside evf_conv2d_wgrad)
        for name, expect, off in (("LeakyFireNet", DETS, {"evf_leaky_bwd", "evf_conv2d_wgrad"}),
                                  ("EVFlowNet BN", {"evf_chan_reduce_det", "evf_conv2d_wgrad_det"}, {"evf_chan_reduce", "evf_conv2d_wgrad"})):
            torch.manual_seed(0)
            model = make_model(name)
            model.train()
            opt = train.FlatAdam(model, lr=2e-4, clip=100.0, device_step=True)
            opts.append(opt)
            opt.zero_grad()
            lossf = EventWarping(LOSS_CFG, DEV)
            step = lambda: train.train_window(model, lossf, opt, win)  # noqa: E731
            _lib.set_deterministic(True)
            assert seen(step) == expect, name
            _lib.set_deterministic(False)
            assert seen(step) == off, name
            _lib.set_deterministic(True)
            assert seen(step) == expect, name

            def forward_on_backward_off():
                model.reset_states()
                _lib.set_deterministic(True)
                out = model(win[0]["event_voxel"], win[0]["event_cnt"])
                _lib.set_deterministic(False)
                sum(f.sum() for f in out["flow"]).backward()

            assert seen(forward_on_backward_off) == expect, name
    finally:
        _lib.set_deterministic(before)
        for opt in opts:
            opt.close()


# ========================================================================================================= the step repeats
def _train(name, sd0, pool, graphed, nsteps=4, warm=2):
    """Two warm-up steps and `nsteps` steps (launched, or replayed from capture_window_cycle's graphs) from the state_dict sd0
    -> (parameters, Adam m, Adam v, recurrent states + norm buffers, losses)."""
    from event_flow_amd.loss.flow import EventWarping
    from event_flow_amd.train import FlatAdam, _general_states, capture_window_cycle, train_window

    model = make_model(name)
    model.load_state_dict(sd0)
    model.train()
    lossf = EventWarping(LOSS_CFG, DEV)
    opt = FlatAdam(model, lr=2e-4, clip=100.0, device_step=True)
    opt.zero_grad()
    start = opt.flat_param.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    losses = []
    with torch.cuda.stream(side):
        for i in range(warm):
            losses.append(train_window(model, lossf, opt, pool[i % 2]).clone())
        torch.cuda.synchronize()
        if graphed:
            graphs, _ = capture_window_cycle(model, lossf, opt, pool, side)
            torch.cuda.synchronize()
        for i in range(nsteps):
            if graphed:
                graphs[i % 2][0].replay()
                torch.cuda.synchronize()
                losses.append(graphs[i % 2][1].clone())
            else:
                losses.append(train_window(model, lossf, opt, pool[i % 2]).clone())
    torch.cuda.synchronize()
    states = [s.clone() for s in _general_states(model)[1]] if name != "EVFlowNet BN" else []
    states += [b.detach().clone() for b in model.buffers()]  # (running mean / variance / batch counter of the batch norms)
    assert float(opt.norm_ws[1]) == warm + nsteps and all(bool(torch.isfinite(x).all()) for x in losses)
    assert float((opt.flat_param - start).abs().max()) > 0
    assert len(states) >= 2 and all(bool(torch.isfinite(s.float()).all()) for s in states)
    out = (opt.flat_param.clone(), opt.m.clone(), opt.v.clone(), states, losses)
    opt.close()
    return out


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "parameters", float((a[0] - b[0]).abs().max()))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (what, "Adam moments")
    assert len(a[3]) == len(b[3]) and len(a[4]) == len(b[4])
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert torch.equal(x, y), (what, "recurrent state / norm buffer", i)
    for i, (x, y) in enumerate(zip(a[4], b[4])):
        assert torch.equal(x, y), (what, "loss of step", i, float(x), float(y))


def _start(name):
    torch.manual_seed(0)
    return copy.deepcopy(make_model(name).state_dict())


@pytest.mark.parametrize("name", ("FireNet", "LeakyFireNet", "EVFlowNet BN", "LIFFireNet k5"))
def test_zoo_steps_repeat_bit_for_bit(det_on, name):
    """2 x 64 x 64, two windows of 3000 events, learning rate 2e-4: two independent eager runs of two warm-up and four steps from
    one state_dict -- parameters, both Adam moments, recurrent states, batch-norm running statistics and every loss torch.equal;
    FireNet (ConvGRU) additionally with the four steps replayed from capture_window_cycle's graphs."""
    pool = windows(2)
    sd0 = _start(name)
    eager = _train(name, sd0, pool, False)
    _same(eager, _train(name, sd0, pool, False), "two eager runs")
    if name == "FireNet":
        _same(eager, _train(name, sd0, pool, True), "graphs against eager")
