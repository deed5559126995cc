"""Deterministic mode on the spiking general path: evf_neuron_bwd_det (the per-channel parameter gradients and g_P of the neuron
backward summed in a fixed order) and evf_clip_adam_step_det (the two-launch optimizer step with a reproducible norm) through
the C ABI against the fp64 references of tests/neuron_gen_ref.py / tests/step_tail_ref.py at the project's own bounds, bit for
bit from call to call, from a NaN-filled scratch and from a captured hipGraph; the host routing behind
EVF_DETERMINISTIC / set_deterministic; and whole training steps of the spiking EV-FlowNets repeated bit for bit.

EVF_DET_GENERAL_REPORT=<file>: the largest observed error of every regime as a fraction of its bound is written there."""

import copy
import os

import numpy as np
import pytest
import torch

import neuron_gen_ref as R
import step_tail_ref as A
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32, F64 = np.float32, np.float64
FILL = 7.0  # initial contents of outputs that a kernel must overwrite (or must leave alone)
PER_ELEMENT = ("g_cur", "g_v_prev", "g_z_prev", "g_aux_prev")
SUMS = ("g_P", "g_p0", "g_p1", "g_p2", "g_p3")

REPORT = {}  # regime -> {output: fraction of its bound}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("EVF_DET_GENERAL_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write(f"bounds: K_E {R.K_E:g}  K_SUM {R.K_SUM:g} (+ chain term), units of 2^-24 * scale; Adam "
                    + "  ".join(f"{k} {v:g}" for k, v in A.BOUND.items()) + "\n")
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
    bound = k * R.U * (np.asarray(scale, F64) + extra).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(frac)) if frac.size else 0
    worst = float(frac[i]) if frac.size else 0.0
    print(f"  {regime} {name}: {worst:.3f} of the bound")
    note(regime, name, worst)
    assert worst <= 1.0, f"{regime} {name}: error {err[i]:.4g} > bound {bound[i]:.4g} at {i}"


# ======================================================================================================== the neuron kernel
def forward(B, case):
    """evf_neuron_fwd -> the saved tensors the backward reads (the device's own v_out / aux_out)."""
    k, n = case["kind"], (case["npix"], case["C"])
    ins = [B.new(a) if a is not None else None for a in (case["cur"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"])]
    prm = [B.new(p) if p is not None else None for p in case["params"]]
    fill = np.full(n, FILL, F32)
    v_out, z_out = B.new(fill), B.new(fill)
    aux_out = B.new(fill) if k != "lif" else None
    rc = call("evf_neuron_fwd", R.KIND_ID[k], P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), None, P(prm[0]), P(prm[1]),
              P(prm[2]), P(prm[3]), case["npix"], case["C"], 1 if case["hard"] else 0, v_out.ptr, z_out.ptr, P(aux_out), None)
    assert rc == 0, (rc, k, n)
    up = {nm: (B.new(a) if a is not None else None) for nm, a in case["upstream"].items()}
    return {"ins": ins, "prm": prm, "v_out": v_out, "aux_out": aux_out, "up": up}


def outputs(B, case, init, null_param=None):
    k, n, prev = case["kind"], (case["npix"], case["C"]), case["prev"]
    fill = np.full(n, FILL, F32)
    o = {"g_cur": B.new(fill)}
    o["g_v_prev"] = B.new(fill) if prev == "present" else None
    # (no gradient for the previous state: g_aux_prev / g_z_prev are handed over all the same and must stay untouched)
    o["g_aux_prev"] = B.new(fill) if (k != "lif" and prev != "absent") else None
    o["g_z_prev"] = B.new(fill) if (k == "alif" and prev != "absent") else None
    o["g_P"] = B.new(np.full(case["npix"], FILL, F32)) if k in ("plif", "xlif") else None
    for i in range(4):
        o[f"g_p{i}"] = B.new(init[i]) if (case["params"][i] is not None and i != null_param) else None
    return o


def backward(entry, case, f, o, ws=None, ws_floats=None):
    """One evf_neuron_bwd / evf_neuron_bwd_det call on the saved tensors of `f` into the buffers `o` -> status."""
    ins, prm, ub = f["ins"], f["prm"], f["up"]
    tail = (P(ws),) if entry == "evf_neuron_bwd" else (P(ws), ws.t.numel() if ws_floats is None else ws_floats)
    return call(entry, R.KIND_ID[case["kind"]], P(ub["g_v_out"]), P(ub["g_z_out"]), P(ub["g_z_out2"]), P(ub["g_aux_out"]),
                f["v_out"].ptr, P(f["aux_out"]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(prm[0]), P(prm[1]), P(prm[2]), P(prm[3]),
                case["npix"], case["C"], 1 if case["hard"] else 0, R.SURROGATE_ID[case["surrogate"]], case["width"], o["g_cur"].ptr,
                P(o["g_v_prev"]), P(o["g_z_prev"]), P(o["g_aux_prev"]), P(o["g_P"]), P(o["g_p0"]), P(o["g_p1"]), P(o["g_p2"]),
                P(o["g_p3"]), *tail)


def det_scratch(B, case, fill=None):
    n = int(_lib.load().evf_neuron_bwd_det_ws(case["npix"], case["C"], R.KIND_ID[case["kind"]]))
    assert n >= R.bwd_geometry(case["C"], case["npix"])["nblk"] * (2 if case["kind"] == "lif" else 4) * case["C"]
    rng = np.random.default_rng(n)
    return B.new(rng.normal(0, 1e3, n).astype(F32) if fill is None else np.full(n, fill, F32))  # (need not be zero on entry)


def init_grads(C, npix):
    rng = np.random.default_rng(C * 7919 + npix)
    return [rng.normal(0, 3, C).astype(F32) for _ in range(4)]  # the parameter gradients are ACCUMULATED onto these


def check_det_backward(regime, case, null_param=None):
    """evf_neuron_bwd_det on the device's own v_out / aux_out: against the fp64 gradients of the update that yields that v_out,
    and its element-wise outputs against evf_neuron_bwd's bits.  -> (buffers, forward, outputs, scratch, initial gradients)."""
    k, C, npix = case["kind"], case["C"], case["npix"]
    B = Bufs()
    f = forward(B, case)
    v32, a32 = f["v_out"].get(), (f["aux_out"].get() if k != "lif" else None)
    ref, sc = R.backward_reference(case, v32, a32)
    init = init_grads(C, npix)
    ws = det_scratch(B, case)
    o = outputs(B, case, init, null_param)
    assert backward("evf_neuron_bwd_det", case, f, o, ws) == 0
    d = outputs(B, case, init, null_param)
    assert backward("evf_neuron_bwd", case, f, d) == 0
    within(regime, "g_cur", o["g_cur"].get(), ref["g_cur"], sc["g_cur"], R.K_E)
    for nm in PER_ELEMENT:
        if o[nm] is None:
            continue
        assert same_bits(o[nm].get(), d[nm].get()), f"{regime}: {nm} differs from evf_neuron_bwd's"
        if nm == "g_cur":
            continue
        if case["prev"] == "present":
            within(regime, nm, o[nm].get(), ref[nm], sc[nm], R.K_E)
        else:
            assert np.all(o[nm].get() == FILL), f"{regime}: {nm} written although the previous state takes no gradient"
    chain, chain_gp = R.chain_terms(C, npix, ws=False)
    if o["g_P"] is not None:
        within(regime, "g_P", o["g_P"].get(), ref["g_P"], sc["g_P"], R.K_SUM + chain_gp)
    for i in range(4):
        if o[f"g_p{i}"] is not None:
            within(regime, f"g_p{i}", o[f"g_p{i}"].get(), ref[f"g_p{i}"] + init[i].astype(F64), sc[f"g_p{i}"], R.K_SUM + chain,
                   extra=np.abs(init[i].astype(F64)))
    B.check()
    return B, f, o, ws, init


def cross():
    from test_gpu_neuron_gen import CROSS

    assert len(CROSS) == 48
    return CROSS


@pytest.mark.parametrize("C,npix", R.SMALL_SHAPES)
def test_det_small_shapes_full_cross(C, npix):
    """4 kinds x hard / soft x upstream state gradient on / off x previous state present / absent / present without a gradient;
    the surrogate cycles with the case; one parameter gradient in turn is null.  The smallest shapes that reach the shuffle arm,
    shuffle + turns, turns, and the arm of a Q that is no power of two."""
    g = R.bwd_geometry(C, npix)
    arm = "not a power of two" if g["np2"] else ("shuffle" if g["Q"] < 64 else ("shuffle + turns" if g["Q"] == 64 else "turns"))
    regime = f"small C={C} npix={npix} (Q={g['Q']}, block {g['bs']}, {arm})"
    for n, (k, hard, gst, prev) in enumerate(cross()):
        check_det_backward(regime, R.make_case(k, C, npix, hard, gst, prev), null_param=n % 5 if n % 5 < 4 else None)


@pytest.mark.parametrize("hard", (True, False))
@pytest.mark.parametrize("kind", ("lif", "xlif"))
@pytest.mark.parametrize("C,npix", R.BLOCK_SHAPES)
def test_det_block_count_regimes_and_repeatability(C, npix, kind, hard):
    """64 blocks with dead tail lanes, 65 / 256, 258 and more, the 1024-block cap with five trips, Q > 64, a Q that is no power of
    two over many blocks -- at the bounds of evf_neuron_bwd.  Then: a second call gives the same bits, a call on a NaN-filled
    scratch too; a scratch one float short, or null, is refused and nothing is written."""
    g = R.bwd_geometry(C, npix)
    regime = f"blocks C={C} npix={npix} {kind} ({g['nblk']} blocks x {g['bs']}, {g['trips']} trips)"
    case = R.make_case(kind, C, npix, hard)
    B, f, first, ws, init = check_det_backward(regime, case)
    again = outputs(B, case, init)
    assert backward("evf_neuron_bwd_det", case, f, again, ws) == 0  # (the scratch as the first call left it)
    nan = outputs(B, case, init)
    assert backward("evf_neuron_bwd_det", case, f, nan, det_scratch(B, case, fill=np.nan)) == 0
    for nm in PER_ELEMENT + SUMS:
        if first[nm] is not None:
            assert same_bits(first[nm].get(), again[nm].get()), f"{regime}: {nm} differs between two calls"
            assert same_bits(first[nm].get(), nan[nm].get()), f"{regime}: {nm} depends on the contents of the scratch"
            assert np.isfinite(first[nm].get()).all()
    untouched = outputs(B, case, init)
    assert backward("evf_neuron_bwd_det", case, f, untouched, ws, ws_floats=ws.t.numel() - 1) == EINVAL
    assert backward("evf_neuron_bwd_det", case, f, untouched, None, ws_floats=ws.t.numel()) == EINVAL
    torch.cuda.synchronize()
    for nm in PER_ELEMENT + ("g_P",):
        if untouched[nm] is not None:
            assert np.all(untouched[nm].get() == FILL), f"{regime}: a refused call wrote {nm}"
    for i in range(2 if kind == "lif" else 4):
        assert same_bits(untouched[f"g_p{i}"].get(), init[i]), f"{regime}: a refused call wrote g_p{i}"
    B.check()


def test_det_refuses_what_the_default_refuses():
    C, npix = 8, 3
    B = Bufs()
    t = [B.new(np.full((npix, 1024), 0.5, F32)) for _ in range(12)]
    p = [B.new(np.full(1028, 0.3, F32)) for _ in range(4)]
    gp = [B.new(np.zeros(1028, F32)) for _ in range(4)]
    Pb, gP = B.new(np.ones(npix, F32)), B.new(np.zeros(npix, F32))
    ws = B.new(np.zeros(4 * 1024 * 4, F32))

    def bwd(kind=0, C=C, P_=Pb.ptr, g_P=gP.ptr, aux_out=t[5].ptr, g_v_prev=t[9].ptr, g_z_prev=t[10].ptr):
        return call("evf_neuron_bwd_det", kind, None, t[7].ptr, None, None, t[4].ptr, aux_out, t[1].ptr, t[2].ptr, t[3].ptr, P_,
                    p[0].ptr, p[1].ptr, p[2].ptr, p[3].ptr, npix, C, 1, 0, 10.0, t[8].ptr, g_v_prev, g_z_prev, t[11].ptr, g_P,
                    gp[0].ptr, gp[1].ptr, gp[2].ptr, gp[3].ptr, ws.ptr, ws.t.numel())

    assert bwd(C=6) == EINVAL and bwd(C=1028) == EINVAL and bwd(C=0) == EINVAL
    assert bwd(kind=4) == EINVAL and bwd(kind=-1) == EINVAL
    assert bwd(kind=1, P_=None) == EINVAL and bwd(kind=3, P_=None) == EINVAL
    assert bwd(kind=1, aux_out=None) == EINVAL and bwd(kind=2, aux_out=None) == EINVAL
    assert bwd(kind=1, g_P=None) == EINVAL and bwd(kind=3, g_P=None) == EINVAL
    assert bwd(kind=2, g_z_prev=None) == EINVAL
    assert bwd(kind=2, g_v_prev=None, g_z_prev=None) == 0  # (no gradient for the previous state: nothing to write)
    for c in range(4, 1025, 4):  # every channel count of the header, every kind
        assert bwd(kind=(c // 4) % 4, C=c) == 0, c
    torch.cuda.synchronize()
    B.check()


# ============================================================================================================ graph replay
@pytest.mark.parametrize("kind,C,npix", (("lif", 32, 33000), ("xlif", 24, 45000), ("xlif", 260, 3100)))
def test_det_calls_replay_from_a_graph_as_they_run_eagerly(kind, C, npix):
    """Two evf_neuron_bwd_det calls, the second accumulating onto the first's parameter gradients, then one evf_clip_adam_step_det
    on those gradients (device-side step counter, zero_grad): captured on a side stream and replayed twice from restored inputs,
    against the same three calls launched eagerly -- bit for bit.  Nothing in between zeroes anything."""
    case = R.make_case(kind, C, npix, True)
    lib = _lib.load()
    n_par = 2 if kind == "lif" else 4
    n = n_par * C
    B = Bufs()
    f = forward(B, case)
    ws = det_scratch(B, case)
    init = np.concatenate(init_grads(C, npix)[:n_par])
    p0 = np.random.default_rng(3).normal(0, 1, n).astype(F32)
    grad, prm, m, v = B.new(init), B.new(p0), B.new(np.zeros(n, F32)), B.new(np.zeros(n, F32))
    nws, part = B.new(np.zeros(8, F32)), B.new(np.full(int(lib.evf_clip_adam_det_ws(n)), np.nan, F32))
    o = outputs(B, case, [init[i * C:(i + 1) * C] for i in range(n_par)] + [None] * (4 - n_par))
    views = [grad.t[i * C:(i + 1) * C] for i in range(n_par)]

    class V:  # the parameter gradients are slices of the flat gradient buffer
        def __init__(self, t):
            self.ptr = t.data_ptr()

    for i in range(n_par):
        o[f"g_p{i}"] = V(views[i])

    def restore():
        grad.set(init), prm.set(p0), m.set(np.zeros(n, F32)), v.set(np.zeros(n, F32)), nws.set(np.zeros(8, F32))
        for nm in PER_ELEMENT + ("g_P",):
            if o[nm] is not None:
                o[nm].t.fill_(FILL)

    def three_calls():
        assert backward("evf_neuron_bwd_det", case, f, o, ws) == 0
        assert backward("evf_neuron_bwd_det", case, f, o, ws) == 0
        assert call("evf_clip_adam_step_det", prm.ptr, grad.ptr, m.ptr, v.ptr, n, 1.0, A.LR, A.B1, A.B2, A.EPS, 0, nws.ptr, 1,
                    part.ptr, part.t.numel()) == 0

    def snapshot():
        torch.cuda.synchronize()
        return {"p": prm.get(), "m": m.get(), "v": v.get(), "ws": nws.get(), "grad": grad.get(),
                **{nm: o[nm].get() for nm in PER_ELEMENT + ("g_P",) if o[nm] is not None}}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        restore()
        three_calls()
        eager = snapshot()
        assert eager["ws"][1] == 1.0 and eager["ws"][0] > 0 and not eager["grad"].any() and np.abs(eager["p"] - p0).max() > 0
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


# ========================================================================================================= optimizer step
def adam_det(n, rg, steps, device_step, zero_grad, shift=0):
    """Teacher-forced steps of evf_clip_adam_step_det against the fp64 reference; every step twice from the same inputs (the
    second time with NaN in the partial sums beforehand): the same bits.  -> worst normalised errors."""
    lib = _lib.load()
    p0, max_norm, gs = A.case_inputs(n, rg)
    B = Bufs()
    zeros = np.zeros(n, F32)
    npart = int(lib.evf_clip_adam_det_ws(n))
    assert min(-(-n // 256), 1024) <= npart <= 1024
    bufs = [[B.new(p0), B.new(zeros), B.new(zeros), B.new(zeros, shift=shift), B.new(np.zeros(8, F32)),
             B.new(np.random.default_rng(n).normal(0, 1e3, npart).astype(F32))] for _ in range(2)]
    p, m, v = p0, zeros, zeros
    worst = dict.fromkeys(("p", "m", "v", "sumsq"), 0.0)
    for t, g in list(enumerate(gs, 1))[:steps]:
        res = []
        for twice, (bp, bm, bv, bg, ws, part) in enumerate(bufs):
            bp.set(p), bm.set(m), bv.set(v), bg.set(g)
            if twice:
                part.set(np.full(npart, np.nan, F32))
            before = ws.get()[1]
            rc = call("evf_clip_adam_step_det", bp.ptr, bg.ptr, bm.ptr, bv.ptr, n, max_norm, A.LR, A.B1, A.B2, A.EPS,
                      0 if device_step else t, ws.ptr, zero_grad, part.ptr, npart)
            assert rc == 0, rc
            w = ws.get()
            assert w[1] == before + (1 if device_step else 0) == (t if device_step else 0), f"step counter {w[1]} after step {t}"
            assert not w.view(np.int32)[2:].any(), f"workspace words 2.. after step {t}: {w}"
            ga = bg.get()
            if zero_grad:
                assert not ga.view(np.int32).any(), "zero_grad = 1 left something in the gradient buffer"
            else:
                assert same_bits(ga, g), "zero_grad = 0 changed the gradient buffer"
            res.append((bp.t.clone(), bm.t.clone(), bv.t.clone(), ws.t[:1].clone()))
        for x, y in zip(*res):
            assert torch.equal(x, y), "two calls from the same inputs differ"
        got = tuple(a.cpu().numpy() for a in res[0][:3])
        e = A.normalised_errors(got + (float(res[0][3]),), (p, m, v), g, max_norm=max_norm, t=t)
        for k in worst:
            worst[k] = max(worst[k], e[k])
            assert e[k] <= A.BOUND[k], f"n={n} {rg} step {t}: {k} error {e[k]:.3g} units > {A.BOUND[k]:.3g} ({e})"
        p, m, v = got
    B.check()
    return worst


@pytest.mark.parametrize("n,shift", ((1, 0), (1023, 0), (4099, 0), ((1 << 20) + 3, 0), (4099, 1)))
def test_adam_det_against_fp64_and_itself(n, shift):
    """One block, the n % 4 tail, several blocks, the 1024-block cap above the fused kernel's limit, and a gradient that is not
    16-byte aligned; the three clip regimes; step counter on the device and from the host, zero_grad on and off."""
    steps = A.STEPS if n <= 4099 else 3  # (teacher-forced: every step is a test of its own; the large size takes three)
    for rg in A.REGIMES:
        for device_step, zero_grad in ((1, 1), (0, 0)):
            worst = adam_det(n, rg, steps, device_step, zero_grad, shift)
            for k, x in worst.items():
                note(f"adam n={n} shift={shift} {rg}", k, x / A.BOUND[k])
        print(f"evf_clip_adam_step_det n={n} shift={shift} {rg}: " + "  ".join(f"{k} {x:.3g}" for k, x in worst.items()))


def test_adam_det_refusals_and_fused_fits():
    lib = _lib.load()
    n = 1025
    B = Bufs()
    b = [B.new(np.full(n, 0.5, F32)) for _ in range(4)]
    ws, part = B.new(np.array([0, 3, 0, 0, 0, 0, 0, 0], F32)), B.new(np.full(int(lib.evf_clip_adam_det_ws(n)), FILL, F32))

    def step(a=(0, 1, 2, 3), n_=n, ws_=ws.ptr, part_=part.ptr, npart=part.t.numel()):
        q = [b[i].ptr if i in a else None for i in range(4)]
        return call("evf_clip_adam_step_det", q[0], q[1], q[2], q[3], n_, 1e-4, A.LR, A.B1, A.B2, A.EPS, 0, ws_, 1, part_, npart)

    for missing in range(4):
        assert step(a=tuple(i for i in range(4) if i != missing)) == EINVAL
    assert step(n_=0) == EINVAL and step(n_=-4) == EINVAL and step(ws_=None) == EINVAL
    assert step(part_=None) == EINVAL and step(npart=part.t.numel() - 1) == EINVAL
    torch.cuda.synchronize()
    assert all(np.all(x.get() == 0.5) for x in b) and ws.get()[1] == 3 and np.all(part.get() == FILL)
    big = torch.empty((1 << 20) + 8, device=DEV)
    assert big.data_ptr() % 16 == 0
    assert lib.evf_clip_adam_fused_fits(1 << 20, big.data_ptr()) == 1
    assert lib.evf_clip_adam_fused_fits((1 << 20) + 1, big.data_ptr()) == 0
    assert lib.evf_clip_adam_fused_fits(1 << 20, big.data_ptr() + 4) == 0
    B.check()


# ================================================================================================================= routing
NEURON_PAIR = ("evf_neuron_bwd", "evf_neuron_bwd_det")
BRACKET = ["evf_neuron_bwd", "evf_neuron_bwd_det", "evf_clip_adam_step", "evf_clip_adam_step_det", "evf_clip_adam_fused"]
LOSS_CFG = {"loader": {"resolution": [64, 64]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def windows(nwin=2, B=2, n=3000, H=64, W=64):
    from event_flow_amd import synthetic
    from event_flow_amd.train import encode_passes

    return [encode_passes([torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 777 + 13 * w)).to(DEV)], 2, (H, W))
            for w in range(nwin)]


def test_the_switch_routes_the_neuron_backward_and_the_optimizer_step(monkeypatch):
    """Profile brackets around one train_window of a SpikingRecEVFlowNet (2 x 64 x 64, 3000 events).  Base 8 has 1.28 M parameters,
    more than the single-launch optimizer step takes (2^20): evf_clip_adam_fused would hand over to the two launches, so with the
    switch on FlatAdam calls evf_clip_adam_step_det.  Base 4 fits: the single launch is reproducible as it stands and stays."""
    from event_flow_amd import train
    from event_flow_amd.loss.flow import EventWarping
    from event_flow_amd.models.model import SpikingRecEVFlowNet
    from test_gpu_general import _unet_cfg

    win = windows(1)[0]

    def make(base):
        torch.manual_seed(0)
        model = SpikingRecEVFlowNet(_unet_cfg(base)).to(DEV)
        model.train()
        opt = train.FlatAdam(model, lr=2e-4, clip=100.0, device_step=True)
        opt.zero_grad()
        return model, EventWarping(LOSS_CFG, DEV), opt

    def seen(fn):
        _lib.profile_start(BRACKET)
        fn()
        return {k[0] for k, v in _lib.profile_stop().items() if v}

    lib = _lib.load()
    before = _lib.deterministic()
    model, lossf, opt = make(8)
    small = make(4)
    step = lambda: train.train_window(model, lossf, opt, win)  # noqa: E731
    try:
        assert lib.evf_clip_adam_fused_fits(opt.n, opt.flat_grad.data_ptr()) == 0
        assert lib.evf_clip_adam_fused_fits(small[2].n, small[2].flat_grad.data_ptr()) == 1
        _lib.set_deterministic(True)
        assert seen(step) == {"evf_neuron_bwd_det", "evf_clip_adam_step_det"}
        assert seen(lambda: train.train_window(*small, win)) == {"evf_neuron_bwd_det", "evf_clip_adam_fused"}
        _lib.set_deterministic(False)
        assert seen(step) == {"evf_neuron_bwd", "evf_clip_adam_fused"}
        monkeypatch.setattr(train, "FUSED_ADAM", False)
        assert seen(step) == {"evf_neuron_bwd", "evf_clip_adam_step"}
        _lib.set_deterministic(True)
        assert seen(step) == {"evf_neuron_bwd_det", "evf_clip_adam_step_det"}
        assert seen(lambda: train.train_window(*small, win)) == {"evf_neuron_bwd_det", "evf_clip_adam_step_det"}

        # a cell follows the switch as it stood in its FORWARD
        def forward_on_backward_off():
            model.reset_states()
            _lib.set_deterministic(True)
            out = model(win[0]["event_voxel"], win[0]["event_cnt"])
            _lib.set_deterministic(False)
            sum(f.sum() for f in out["flow"]).backward()

        assert seen(forward_on_backward_off) & set(NEURON_PAIR) == {"evf_neuron_bwd_det"}
    finally:
        _lib.set_deterministic(before)
        opt.close()
        small[2].close()


# ========================================================================================================= the step repeats
LIF_NEURON = {"leak": [-4.0, 0.1], "thresh": [0.3, 0.05], "learn_leak": True, "learn_thresh": True, "hard_reset": True}
XLIF_NEURON = {"leak_v": [-4.0, 0.1], "leak_pt": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
               "learn_thresh": True, "hard_reset": True}  # (the values of tests/test_gpu_deterministic.py)
THRESH_SCALE = {"SpikingRecEVFlowNet": 1.0, "XLIFRecEVFlowNet": 0.25}  # (XLIF: t0 and t1 scaled so that every layer spikes)


def _unet(name, neuron):
    from event_flow_amd.models import model as models

    cfg = {"num_bins": 2, "base_num_channels": 8, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
           "activations": ["arctanspike", "arctanspike"], "spiking_neuron": dict(neuron)}
    return getattr(models, name)(cfg).to(DEV)


def _train(name, neuron, sd0, pool, graphed, nsteps=4, warm=2):
    """Two warm-up steps and `nsteps` steps (launched, or replayed from capture_window_cycle's graphs) from the state_dict sd0
    -> (parameters, Adam m, Adam v, recurrent states, losses)."""
    from event_flow_amd.loss.flow import EventWarping
    from event_flow_amd.train import FlatAdam, _general_states, capture_window_cycle, train_window

    model = _unet(name, neuron)
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
            graphs, copied = capture_window_cycle(model, lossf, opt, pool, side, route=True)
            assert copied == 0
            torch.cuda.synchronize()
        for i in range(nsteps):
            if graphed:
                graphs[i % 2][0].replay()
                torch.cuda.synchronize()
                losses.append(graphs[i % 2][1].clone())
            else:
                losses.append(train_window(model, lossf, opt, pool[i % 2]).clone())
    torch.cuda.synchronize()
    states = [s.clone() for s in _general_states(model)[1]]
    # it trained: the parameters moved, the step counter ran, every layer spiked in the last pass
    assert float(opt.norm_ws[1]) == warm + nsteps and all(bool(torch.isfinite(x).all()) for x in losses)
    assert float((opt.flat_param - start).abs().max()) > 0
    assert len(states) >= 8 and all(float(s[1].abs().sum()) > 0 for s in states), [float(s[1].abs().sum()) for s in states]
    out = (opt.flat_param.clone(), opt.m.clone(), opt.v.clone(), states, losses)
    opt.close()
    return out


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "parameters", float((a[0] - b[0]).abs().max()))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (what, "Adam moments")
    assert len(a[3]) == len(b[3]) and len(a[4]) == len(b[4])
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert torch.equal(x, y), (what, "recurrent state", i)
    for i, (x, y) in enumerate(zip(a[4], b[4])):
        assert torch.equal(x, y), (what, "loss of step", i, float(x), float(y))


def _start(name, neuron):
    torch.manual_seed(0)
    first = _unet(name, neuron)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith(("thresh", "t0", "t1")):
                p.mul_(THRESH_SCALE[name])
    return copy.deepcopy(first.state_dict())


def test_lif_evflownet_steps_repeat_bit_for_bit_eagerly_and_from_graphs(det_on):
    """The configuration of test_general_path_window_cycle_replays_without_state_copies (2 x 64 x 64, base 8, thresh 0.3, two
    windows of 3000 events) WITH a learning rate: (a) two independent eager runs of two warm-up and four steps from one
    state_dict, (b) the four steps replayed from capture_window_cycle's routed graphs -- parameters, both Adam moments, every
    recurrent state tensor and every loss torch.equal."""
    pool = windows(2)
    sd0 = _start("SpikingRecEVFlowNet", LIF_NEURON)
    eager1 = _train("SpikingRecEVFlowNet", LIF_NEURON, sd0, pool, False)
    eager2 = _train("SpikingRecEVFlowNet", LIF_NEURON, sd0, pool, False)
    _same(eager1, eager2, "two eager runs")
    _same(eager1, _train("SpikingRecEVFlowNet", LIF_NEURON, sd0, pool, True), "graphs against eager")


def test_xlif_evflownet_steps_repeat_bit_for_bit(det_on):
    """(a) for the XLIF EV-FlowNet: g_P and the pre-synaptic trace's gradient path."""
    pool = windows(2)
    sd0 = _start("XLIFRecEVFlowNet", XLIF_NEURON)
    _same(_train("XLIFRecEVFlowNet", XLIF_NEURON, sd0, pool, False), _train("XLIFRecEVFlowNet", XLIF_NEURON, sd0, pool, False),
          "two eager runs")
