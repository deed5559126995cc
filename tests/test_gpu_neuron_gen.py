"""The element-wise kernels of the general path (csrc/evf_neuron_gen.hip) through the C ABI against the plain references of
tests/neuron_gen_ref.py: evf_neuron_fwd / evf_neuron_bwd over every channel-reduction arm and block-count regime of the backward
(spikes bit for bit, everything else within the bounds that tests/test_host_neuron_gen_reference.py establishes on the CPU),
evf_lif_fwd_parts bit for bit against evf_neuron_fwd, evf_leaky_fwd / _bwd and evf_pretrace_fwd / _bwd within bounds worked out
from their arithmetic.  Every buffer handed to a kernel sits between 64 guard elements on either side.

EVF_NEURON_GEN_REPORT=<file>: the largest observed error of every regime as a fraction of its bound is written there."""

import os

import numpy as np
import pytest
import torch

import neuron_gen_ref as R
from event_flow_amd import _lib
from gpu_bufs import Bufs

pytestmark = pytest.mark.gpu
EINVAL = -22
F32, F64 = np.float32, np.float64
WS_FLOATS = 32 * 4096 + 64  # EVF_NEURON_BWD_WS
FILL = 7.0  # initial contents of outputs that a kernel must overwrite (or must leave alone)

REPORT = {}  # regime -> {"worst": {output: fraction of its bound}, "spikes": mismatches, "cases": n}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("EVF_NEURON_GEN_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write(f"bounds: K_E {R.K_E:g}  K_SUM {R.K_SUM:g} (+ chain term)  K_LEAKY {R.K_LEAKY:g}; units of 2^-24 * scale\n")
            for regime, r in REPORT.items():
                worst = "  ".join(f"{k} {v:.3f}" for k, v in sorted(r["worst"].items()))
                head = f"cases {r['cases']}  spike mismatches {r['spikes']}  " if r["cases"] else ""
                f.write(f"{regime}: {head}error / bound: {worst}\n")


def note(regime, name, frac):
    r = REPORT.setdefault(regime, {"worst": {}, "spikes": 0, "cases": 0})
    r["worst"][name] = max(r["worst"].get(name, 0.0), float(frac))


def call(name, *args):
    return _lib.raw(name, *args)


def P(b):
    return None if b is None else b.ptr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def within(regime, name, got, ref, scale, k, extra=0.0):
    """|got - ref| <= k * 2^-24 * (scale + extra) everywhere; records the fraction of the bound that was used."""
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64)).reshape(-1)
    bound = k * R.U * (np.asarray(scale, F64) + extra).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(frac)) if frac.size else 0
    worst = float(frac[i]) if frac.size else 0.0
    print(f"  {regime} {name}: {worst:.3f} of the bound")
    note(regime, name, worst)
    assert worst <= 1.0, f"{regime} {name}: error {err[i]:.4g} > bound {bound[i]:.4g} at {i} (got {np.asarray(got).reshape(-1)[i]}, ref {np.asarray(ref).reshape(-1)[i]})"


# ======================================================================================================= neuron fwd / bwd
def neuron_forward(B, case, *, residual=True, out=True):
    k = case["kind"]
    n = (case["npix"], case["C"])
    ins = [B.new(a) if a is not None else None for a in (case["cur"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"])]
    res = B.new(case["residual"]) if residual else None
    prm = [B.new(p) if p is not None else None for p in case["params"]]
    fill = np.full(n, FILL, F32)
    v_out, z_out = B.new(fill), B.new(fill)
    aux_out = B.new(fill) if k != "lif" else None
    o = B.new(fill) if out else None
    rc = call("evf_neuron_fwd", R.KIND_ID[k], P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(res), P(prm[0]), P(prm[1]),
              P(prm[2]), P(prm[3]), case["npix"], case["C"], 1 if case["hard"] else 0, v_out.ptr, z_out.ptr, P(aux_out), P(o))
    assert rc == 0, (rc, k, n)
    return {"ins": ins, "prm": prm, "v_out": v_out, "z_out": z_out, "aux_out": aux_out, "out": o}


def check_forward(regime, case, variants=True):
    """evf_neuron_fwd against the fp64 reference; -> the buffers of the call (v_out / aux_out feed the backward)."""
    B = Bufs()
    k = case["kind"]
    f = neuron_forward(B, case)
    ref = case["ref_fwd"]
    z, o, v = f["z_out"].get(), f["out"].get(), f["v_out"].get()
    bad = int(np.count_nonzero(z != ref["z_out"]) + np.count_nonzero(o != ref["out"]))
    REPORT.setdefault(regime, {"worst": {}, "spikes": 0, "cases": 0})
    REPORT[regime]["spikes"] += bad
    REPORT[regime]["cases"] += 1
    assert bad == 0, f"{regime}: {bad} spike / output mismatches"
    assert same_bits(z, ref["z_out"]) and same_bits(o, ref["out"])
    fs = R.forward_scales(k, case["cur"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], case["params"], case["hard"])
    within(regime, "v_out", v, ref["v_out"], fs["v_out"], R.K_E)
    if k != "lif":
        within(regime, "aux_out", f["aux_out"].get(), ref["aux_out"], fs["aux_out"], R.K_E)
    if variants:
        # out null and out given agree; without a residual the output IS the spike tensor
        for kw in ({"out": False}, {"residual": False}):
            g = neuron_forward(B, case, **kw)
            assert same_bits(g["v_out"].get(), v) and same_bits(g["z_out"].get(), z), kw
            if k != "lif":
                assert same_bits(g["aux_out"].get(), f["aux_out"].get()), kw
            if g["out"] is not None:
                assert same_bits(g["out"].get(), z), kw
    B.check()
    return B, f


def neuron_backward(B, case, f, ws, init, null_param=None):
    """One evf_neuron_bwd call on the saved tensors of the forward `f` -> output buffers."""
    k, n = case["kind"], (case["npix"], case["C"])
    up = case["upstream"]
    ub = {nm: (B.new(a) if a is not None else None) for nm, a in up.items()}
    fill = np.full(n, FILL, F32)
    o = {"g_cur": B.new(fill)}
    prev = case["prev"]
    o["g_v_prev"] = B.new(fill) if prev == "present" else None
    # (no gradient for the previous state: g_aux_prev / g_z_prev are handed over all the same and must stay untouched)
    o["g_aux_prev"] = B.new(fill) if (k != "lif" and prev != "absent") else None
    o["g_z_prev"] = B.new(fill) if (k == "alif" and prev != "absent") else None
    o["g_P"] = B.new(np.full(case["npix"], FILL, F32)) if k in ("plif", "xlif") else None
    for i in range(4):
        have = case["params"][i] is not None and i != null_param
        o[f"g_p{i}"] = B.new(init[i]) if have else None
    ins, prm = f["ins"], f["prm"]
    rc = call("evf_neuron_bwd", R.KIND_ID[k], P(ub["g_v_out"]), P(ub["g_z_out"]), P(ub["g_z_out2"]), P(ub["g_aux_out"]),
              f["v_out"].ptr, P(f["aux_out"]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(prm[0]), P(prm[1]), P(prm[2]), P(prm[3]),
              case["npix"], case["C"], 1 if case["hard"] else 0, R.SURROGATE_ID[case["surrogate"]], case["width"], o["g_cur"].ptr,
              P(o["g_v_prev"]), P(o["g_z_prev"]), P(o["g_aux_prev"]), P(o["g_P"]), P(o["g_p0"]), P(o["g_p1"]), P(o["g_p2"]),
              P(o["g_p3"]), P(ws))
    assert rc == 0, (rc, k, n)
    return o


def check_backward(regime, case, B, f, *, ws_modes=("ws",), null_param=None):
    """evf_neuron_bwd on the device's own v_out / aux_out against the fp64 gradients of the update that yields that v_out."""
    k, C, npix = case["kind"], case["C"], case["npix"]
    v32, a32 = f["v_out"].get(), (f["aux_out"].get() if k != "lif" else None)
    ref, sc = R.backward_reference(case, v32, a32)
    rng = np.random.default_rng(C * 7919 + npix)
    init = [rng.normal(0, 3, C).astype(F32) for _ in range(4)]  # the parameter gradients are ACCUMULATED onto these
    ws = B.new(np.zeros(WS_FLOATS, F32))
    geom = R.bwd_geometry(C, npix)
    for mode in ws_modes:
        o = neuron_backward(B, case, f, None if mode == "null" else ws, init, null_param)
        tag = regime if mode == "ws" else f"{regime} [{mode}]"
        within(tag, "g_cur", o["g_cur"].get(), ref["g_cur"], sc["g_cur"], R.K_E)
        for nm in ("g_v_prev", "g_z_prev", "g_aux_prev"):
            if o[nm] is None:
                continue
            if case["prev"] == "present":
                within(tag, nm, o[nm].get(), ref[nm], sc[nm], R.K_E)
            else:
                assert np.all(o[nm].get() == FILL), f"{tag}: {nm} written although the previous state takes no gradient"
        chain, chain_gp = R.chain_terms(C, npix, ws=mode != "null")
        if o["g_P"] is not None:
            within(tag, "g_P", o["g_P"].get(), ref["g_P"], sc["g_P"], R.K_SUM + chain_gp)
        for i in range(4):
            if o[f"g_p{i}"] is not None:
                within(tag, f"g_p{i}", o[f"g_p{i}"].get(), ref[f"g_p{i}"] + init[i].astype(F64), sc[f"g_p{i}"], R.K_SUM + chain,
                       extra=np.abs(init[i].astype(F64)))
        w = ws.get()
        assert not w.view(np.int32).any(), f"{tag}: the scratch (ticket word included) is not zero after the call"
    assert geom["replicas"] or ws_modes == ("ws",)
    B.check()


CROSS = [(k, hard, gst, prev) for k in R.KINDS for hard in (True, False) for gst in (True, False) for prev in R.PREV_MODES]


@pytest.mark.parametrize("C,npix", R.SMALL_SHAPES)
def test_neuron_small_shapes_full_cross(C, npix):
    """4 kinds x hard / soft x upstream state gradient on / off x previous state present / absent / present without a gradient;
    the surrogate cycles with the case; one parameter gradient in turn is null."""
    g = R.bwd_geometry(C, npix)
    arm = "not a power of two" if g["np2"] else ("shuffle" if g["Q"] < 64 else ("shuffle + turns" if g["Q"] == 64 else "turns"))
    regime = f"small C={C} npix={npix} (Q={g['Q']}, block {g['bs']}, {arm})"
    for n, (k, hard, gst, prev) in enumerate(CROSS):
        case = R.make_case(k, C, npix, hard, gst, prev)
        B, f = check_forward(regime, case)
        check_backward(regime, case, B, f, null_param=n % 5 if n % 5 < 4 else None)


@pytest.mark.parametrize("hard", (True, False))
@pytest.mark.parametrize("kind", ("lif", "xlif"))
@pytest.mark.parametrize("C,npix", R.BLOCK_SHAPES)
def test_neuron_block_count_regimes(C, npix, kind, hard):
    """Both resets, state gradient and previous state present.  On the replica path: the scratch comes back zeroed, a second call on
    the same scratch and a call without scratch stay within the same bounds."""
    g = R.bwd_geometry(C, npix)
    regime = f"blocks C={C} npix={npix} ({g['nblk']} blocks x {g['bs']}, {g['trips']} trips, {'replicas' if g['replicas'] else 'direct'})"
    case = R.make_case(kind, C, npix, hard)
    B, f = check_forward(regime, case, variants=False)
    check_backward(regime, case, B, f, ws_modes=("ws", "ws again", "null") if g["replicas"] else ("ws",))


def test_neuron_real_valued_previous_spikes():
    """Group-norm cells hand NORMALISED spikes to the reset: z_prev is any real number."""
    for hard in (True, False):
        case = R.make_case("lif", 32, 70, hard, True, "present", True)
        assert np.count_nonzero((case["z_prev"] != 0) & (case["z_prev"] != 1)) > 2000
        B, f = check_forward("real-valued z_prev", case)
        check_backward("real-valued z_prev", case, B, f)


# ============================================================================================================== lif parts
@pytest.mark.parametrize("C,npix", ((32, 70), (24, 33), (1024, 4100)))
def test_lif_fwd_parts_equals_neuron_fwd_on_the_summed_current(C, npix):
    """cur = (a[0] + a[1] + ...) and, with a recurrent part, (b[0] + b[1] + ...) + that: plain fp32 adds in index order, so the
    result equals evf_neuron_fwd(LIF) on the numpy sum BIT FOR BIT.  Slab strides larger than the tensor."""
    n = npix * C
    rng = np.random.default_rng(C + npix)
    case = R.make_case("lif", C, npix, True)
    for na in (1, 2, 5):
        for nb in (None, 1, 3):
            hard = (na + (nb or 0)) % 2
            sa, sb = n + 4 * na, n + 4 * (nb or 0) + 8
            a = rng.uniform(-3, 3, (na, sa)).astype(F32)
            b = rng.uniform(-3, 3, (nb, sb)).astype(F32) if nb else None
            cur = a[0, :n].copy()
            for z in range(1, na):
                cur += a[z, :n]
            if nb:
                d = b[0, :n].copy()
                for z in range(1, nb):
                    d += b[z, :n]
                cur = d + cur
            B = Bufs()
            ab, bb = B.new(a), (B.new(b) if nb else None)
            cb = B.new(cur)
            vp, zp, res = B.new(case["v_prev"]), B.new(case["z_prev"]), B.new(case["residual"])
            lk, th = B.new(case["params"][0]), B.new(case["params"][1])
            fill = np.full(n, FILL, F32)
            outs = [[B.new(fill) for _ in range(3)] for _ in range(2)]
            rc = call("evf_lif_fwd_parts", ab.ptr, na, sa, P(bb), nb or 0, sb, vp.ptr, zp.ptr, res.ptr, lk.ptr, th.ptr, npix, C, hard,
                      outs[0][0].ptr, outs[0][1].ptr, outs[0][2].ptr)
            assert rc == 0
            rc = call("evf_neuron_fwd", 0, cb.ptr, vp.ptr, zp.ptr, None, None, res.ptr, lk.ptr, th.ptr, None, None, npix, C, hard,
                      outs[1][0].ptr, outs[1][1].ptr, None, outs[1][2].ptr)
            assert rc == 0
            for x, y, nm in zip(outs[0], outs[1], ("v_out", "z_out", "out")):
                assert same_bits(x.get(), y.get()), (nm, na, nb)
            assert not np.any(outs[0][0].get() == FILL)
            B.check()


# ================================================================================================================== leaky
def leaky_chain(C, npix):
    """Adds a term of g_leak can pass through: a thread's trips, the block's LDS word (every thread of the channel quad), the
    replica (blocks / 32), the 32 replicas, the output."""
    Q = C // 4
    bs = 256 if Q >= 256 else (256 // Q) * Q
    total = npix * Q
    nblk = min(-(-total // bs), 1024)
    return -(-total // (nblk * bs)) + bs // Q + -(-nblk // 32) + 32 + 1


@pytest.mark.parametrize("C,npix", ((8, 70), (24, 33), (260, 7), (32, 40000)))
def test_leaky_forward_and_backward(C, npix):
    """Four activations; prev, residual, g_out and g_state each present and absent; g_leak accumulated onto non-zero contents and
    null; every backward TWICE, because the replica array is a device global that must come back zeroed."""
    rng = np.random.default_rng(C * 31 + npix)
    n = (npix, C)
    regime = f"leaky C={C} npix={npix}"
    u = lambda: rng.uniform(-2, 2, n).astype(F32)  # noqa: E731
    cur, prev, res, g_out, g_state = u(), u(), u(), rng.normal(0, 1, n).astype(F32), rng.normal(0, 1, n).astype(F32)
    leak = rng.uniform(-4, 4, C).astype(F32)
    init = rng.normal(0, 3, C).astype(F32)
    chain = leaky_chain(C, npix)
    big = npix > 1000
    combos = [(p, r, go, gs) for p in (1, 0) for r in (1, 0) for go in (1, 0) for gs in (1, 0) if go or gs]
    if big:
        combos = [(1, 1, 1, 1), (0, 0, 1, 0)]
    for act_id, act in enumerate(R.ACTS):
        for has_prev, has_res, has_go, has_gs in combos:
            B = Bufs()
            cb, lb = B.new(cur), B.new(leak)
            pb = B.new(prev) if has_prev else None
            rb = B.new(res) if has_res else None
            fill = np.full(n, FILL, F32)
            mix, out = B.new(fill), B.new(fill)
            assert call("evf_leaky_fwd", cb.ptr, P(pb), P(rb), lb.ptr, act_id, npix, C, mix.ptr, out.ptr) == 0
            ref = R.leaky_ref(cur, prev if has_prev else None, res if has_res else None, leak, act)
            within(regime, "mix", mix.get(), ref["mix"], ref["s_mix"], R.K_LEAKY)
            within(regime, "out", out.get(), ref["out"], ref["s_out"], R.K_LEAKY)
            mix2 = B.new(fill)
            assert call("evf_leaky_fwd", cb.ptr, P(pb), P(rb), lb.ptr, act_id, npix, C, mix2.ptr, None) == 0
            assert same_bits(mix2.get(), mix.get())
            # backward on the device's own mix: the reference differentiates the update that yields exactly that mix
            m32 = mix.get().astype(F64)
            lam = 1 / (1 + np.exp(-leak.astype(F64)))
            cur_rec = (m32 - (prev.astype(F64) if has_prev else 0.0) * lam) / (1 - lam)
            go, gs = (g_out if has_go else None), (g_state if has_gs else None)
            bref = R.leaky_ref(cur_rec, prev if has_prev else None, None, leak, act, g_out=go, g_state=gs)
            gob, gsb = (B.new(go) if has_go else None), (B.new(gs) if has_gs else None)
            g_leak = B.new(init)
            for rep in (1, 2):
                g_cur, g_prev = B.new(fill), B.new(fill)
                assert call("evf_leaky_bwd", P(gob), P(gsb), mix.ptr, P(pb), lb.ptr, act_id, npix, C, g_cur.ptr, g_prev.ptr,
                            g_leak.ptr) == 0
                within(regime, "g_cur", g_cur.get(), bref["g_cur"], bref["s_g_cur"], R.K_LEAKY)
                within(regime, "g_prev", g_prev.get(), bref["g_prev"], bref["s_g_prev"], R.K_LEAKY)
                within(regime, "g_leak", g_leak.get(), init.astype(F64) + rep * bref["g_leak"], rep * bref["s_g_leak"],
                       R.K_LEAKY + chain + rep, extra=np.abs(init.astype(F64)))
            g_cur = B.new(fill)
            assert call("evf_leaky_bwd", P(gob), P(gsb), mix.ptr, P(pb), lb.ptr, act_id, npix, C, g_cur.ptr, None, None) == 0
            within(regime, "g_cur", g_cur.get(), bref["g_cur"], bref["s_g_cur"], R.K_LEAKY)
            B.check()


def test_leaky_refusals():
    B = Bufs()
    x = B.new(np.zeros((3, 8), F32))
    lk = B.new(np.zeros(8, F32))
    assert call("evf_leaky_fwd", x.ptr, None, None, lk.ptr, 4, 3, 8, x.ptr, None) == EINVAL
    assert call("evf_leaky_fwd", x.ptr, None, None, lk.ptr, 0, 4, 6, x.ptr, None) == EINVAL
    assert call("evf_leaky_bwd", None, None, x.ptr, None, lk.ptr, 0, 3, 8, x.ptr, None, None) == EINVAL
    B.check()


# =============================================================================================================== pretrace
@pytest.mark.parametrize("C", (2, 4, 6, 20, 64, 130))
def test_pretrace_forward_and_backward(C):
    """P = avg_pool2d(mean_c |x|) and its adjoint: kernel sizes 3 / 5 / 7, strides 1 / 2, pixel strides larger than C, three
    image sizes (a single row, a single column), accumulate 0 / 1, zeros in x (sign 0).
    Bounds: a pixel's mean is a sum of non-negative terms -- C / tpp adds per lane (tpp <= 64 lanes per pixel) and log2(tpp)
    shuffle levels, one divide; the pool adds k^2 of them and divides: (C / tpp + 6 + k^2 + 2) roundings of the (non-negative)
    result.  Backward: k^2 adds, two divides, one add onto the previous contents."""
    regime = f"pretrace C={C}"
    rng = np.random.default_rng(C)
    ldx, ldg = C + 3, C + 5
    tpp = min(64, 1 << int(np.floor(np.log2(C))))
    for (Bn, H, W) in ((2, 7, 9), (1, 1, 5), (1, 12, 1)):
        x = rng.normal(0, 1, (Bn, H, W, C)).astype(F32)
        x[rng.random(x.shape) < 0.15] = 0.0
        xs = np.full((Bn, H, W, ldx), FILL, F32)
        xs[..., :C] = x
        for k in (3, 5, 7):
            for s in (1, 2):
                Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
                g_P = rng.normal(0, 1, (Bn, Ho, Wo)).astype(F32)
                ref = R.pretrace_ref(x, k, s, g_P=g_P)
                assert ref["P"].shape == (Bn, Ho, Wo)
                B = Bufs()
                xb, ws, Pb = B.new(xs), B.new(np.full(Bn * H * W, FILL, F32)), B.new(np.full((Bn, Ho, Wo), FILL, F32))
                assert call("evf_pretrace_fwd", xb.ptr, ldx, Bn, H, W, C, k, s, ws.ptr, Pb.ptr) == 0
                within(regime, "P", Pb.get(), ref["P"], ref["P"], -(-C // tpp) + 6 + k * k + 2)
                gb = B.new(g_P)
                for accumulate in (0, 1):
                    init = rng.normal(0, 1, (Bn, H, W, ldg)).astype(F32)
                    gx = B.new(init)
                    assert call("evf_pretrace_bwd", xb.ptr, ldx, gb.ptr, Bn, H, W, C, k, s, gx.ptr, ldg, accumulate) == 0
                    got = gx.get()
                    assert same_bits(got[..., C:], init[..., C:]), "wrote between the pixels"
                    before = init[..., :C].astype(F64) if accumulate else 0.0
                    within(regime, "g_x", got[..., :C], before + ref["g_x"], ref["s_g_x"], k * k + 3, extra=np.abs(before))
                    assert np.all((got[..., :C] == (init[..., :C] if accumulate else 0))[x == 0]), "sign(0) is 0"
                B.check()


# ============================================================================================================== refusals
def test_neuron_refusals_and_every_channel_count():
    C, npix = 8, 3
    B = Bufs()
    t = [B.new(np.full((npix, 1024), 0.5, F32)) for _ in range(12)]
    p = [B.new(np.full(1028, 0.3, F32)) for _ in range(4)]
    gp = [B.new(np.zeros(1028, F32)) for _ in range(4)]
    Pb, gP = B.new(np.ones(npix, F32)), B.new(np.zeros(npix, F32))

    def fwd(kind=0, C=C, P_=Pb.ptr, aux_out=t[5].ptr):
        return call("evf_neuron_fwd", kind, t[0].ptr, t[1].ptr, t[2].ptr, t[3].ptr, P_, None, p[0].ptr, p[1].ptr, p[2].ptr,
                    p[3].ptr, npix, C, 1, t[4].ptr, t[6].ptr, aux_out, None)

    def bwd(kind=0, C=C, P_=Pb.ptr, g_P=gP.ptr, aux_out=t[5].ptr, g_v_prev=t[9].ptr, g_z_prev=t[10].ptr):
        return call("evf_neuron_bwd", kind, None, t[7].ptr, None, None, t[4].ptr, aux_out, t[1].ptr, t[2].ptr, t[3].ptr, P_,
                    p[0].ptr, p[1].ptr, p[2].ptr, p[3].ptr, npix, C, 1, 0, 10.0, t[8].ptr, g_v_prev, g_z_prev, t[11].ptr, g_P,
                    gp[0].ptr, gp[1].ptr, gp[2].ptr, gp[3].ptr, None)

    for f in (fwd, bwd):
        assert f(C=6) == EINVAL and f(C=1028) == EINVAL and f(C=0) == EINVAL
        assert f(kind=4) == EINVAL and f(kind=-1) == EINVAL
        assert f(kind=1, P_=None) == EINVAL and f(kind=3, P_=None) == EINVAL
        assert f(kind=1, aux_out=None) == EINVAL and f(kind=2, aux_out=None) == EINVAL
    assert bwd(kind=1, g_P=None) == EINVAL and bwd(kind=3, g_P=None) == EINVAL
    assert bwd(kind=2, g_z_prev=None) == EINVAL
    assert bwd(kind=2, g_v_prev=None, g_z_prev=None) == 0  # (no gradient for the previous state: nothing to write)
    # the header promises C % 4 == 0 up to 1024, forward AND backward, for every kind
    for c in range(4, 1025, 4):
        kind = (c // 4) % 4
        assert fwd(kind=kind, C=c) == 0, c
        assert bwd(kind=kind, C=c) == 0, c
    torch.cuda.synchronize()
    B.check()
