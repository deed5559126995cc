"""References for the element-wise kernels of the general path (csrc/evf_neuron_gen.hip): evf_neuron_fwd / evf_neuron_bwd /
evf_lif_fwd_parts, evf_leaky_fwd / _bwd, evf_pretrace_fwd / _bwd.  Plain torch and numpy, dtype preserving (fp64 by default).

Shared by tests/test_host_neuron_gen_reference.py (which ties the reference to oracle.snn, measures the bounds below without
a GPU and shows that they reject eight ways of getting the backward subtly wrong) and tests/test_gpu_neuron_gen.py (which
holds the kernels to them).  Not a test module itself.

Layout: tensors [npix][C], P [npix], parameters [C] (slots p0..p3 as in include/evflow.h).

What crosses the C ABI as `float` is rounded to fp32 FIRST in every reference: the surrogate width, and the clamp constant
0.01f -- a threshold parameter of fp32(0.01) sits exactly AT the clamp for the kernels (and for torch in fp32) but below the
double 0.01.

Errors are measured in units of 2^-24 * scale, where the scale of an output is its own expression with every product
replaced by the product of the absolute values and every sum by the sum of the absolute values (neuron_scales, written out
by hand).  The backward recovers the input current from the saved v_out, cur = (v_out - reset term) / (1 - lam): the
scale of everything that reads it carries that quotient, not |cur|.
"""

import functools

import numpy as np
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit round-off of fp32

KINDS = ("lif", "plif", "alif", "xlif")
KIND_ID = {k: i for i, k in enumerate(KINDS)}
SURROGATES = ("arctanspike", "superspike", "trianglespike", "mgspike")
SURROGATE_ID = dict(zip(SURROGATES, range(4)))  # EVF_ARCTAN, EVF_SUPERSPIKE, EVF_TRIANGLE, EVF_MULTIGAUSS
# widths at which every surrogate is non-zero over a good part of |v - thresh| <= 8 (all exact in fp32)
WIDTH = {"arctanspike": 10.0, "superspike": 10.0, "trianglespike": 0.25, "mgspike": 0.5}
CLAMP1 = float(F32(0.01))  # thresh / t0 .clamp_min(0.01) as the kernels (and torch in fp32) see the constant
MARGIN = 1e-4  # no fp64 v_out of a generated case lies closer to its threshold

PER_ELEMENT = ("g_cur", "g_v_prev", "g_z_prev", "g_aux_prev")
PARAM_SUMS = ("g_p0", "g_p1", "g_p2", "g_p3")

MUTANTS = ("clamp_mask_gt", "soft_reset_new_trace", "z_not_detached", "alif_g_z_prev_dropped", "g_P_without_one_minus_leak",
           "g_z_out2_ignored", "t1_without_gsoft_term", "last_pixel_dropped")

# ---- bounds (units of 2^-24 * scale) --------------------------------------------------------------------------------------
# Measured: the worst error of emulate32 (fp32, the kernels' operation order) against neuron_ref in fp64 over the full cross
# of the small cases (SMALL_SHAPES x kinds x resets x state gradient x previous state; tests/test_host_neuron_gen_reference.py
# prints them and checks that the figures below are the measured ones):
#     per element (v_out, aux_out, g_cur, g_v_prev, g_z_prev, g_aux_prev)   MEASURED["element"]
#     parameter sums and g_P (sums over pixels / channels)                   MEASURED["sum"]
# Bound = 4 x measured.  The factor covers what the emulation does not share with the device: its expf (the emulation's is
# numpy's), and another order of the sums.  On top of K_SUM a sum gets the chain term of its launch geometry (chain_terms).
#     element 10.09 (g_aux_prev; v_out 3.96, g_cur 7.45, g_v_prev 8.63)   sum 53.31 (g_p2; g_p3 48.4, g_p1 12.3, g_p0 5.9, g_P 5.7)
# The sums' figure is the factor a (1 - a) of a sigmoid-valued parameter behind the sum: at a logit of 4, 1 - a = 0.018 carries
# the rounding of a, 55 times larger relative to itself.  Recorded rounded up by 4 % (another libm's exp moves them a little).
MEASURED = {"element": 10.5, "sum": 55.0}
K_E = 4.0 * MEASURED["element"]
K_SUM = 4.0 * MEASURED["sum"]

SMALL_SHAPES = ((4, 5), (8, 70), (32, 70), (128, 9), (256, 5), (260, 7), (384, 5), (1024, 3),
                (12, 70), (24, 33), (48, 17), (132, 6), (252, 5))  # the last five: Q = C / 4 below 64, not a power of two
# block-count regimes of evf_neuron_bwd (bwd_geometry): 64 blocks of three trips with dead tail lanes; 65 and 256 blocks adding
# straight into the outputs; the 32 replicas from 258 blocks on; the 1024-block cap with five trips (the forward's 4096-block
# cap too); the replicas behind each wide-channel reduction and behind a Q that is not a power of two
BLOCK_SHAPES = ((32, 4097), (32, 8200), (32, 32768), (32, 33000), (32, 140000), (256, 4100), (260, 3100), (384, 2100), (1024, 1100),
                (24, 45000))
PREV_MODES = ("present", "absent", "no_g_prev")


# ------------------------------------------------------------------------------------------------------------- surrogates
def _gauss(x, mu, sigma):
    return torch.exp(-((x - mu) * (x - mu)) / (2 * sigma * sigma)) / (sigma * float(np.sqrt(2 * np.pi)))


def surrogate_ref(kind, x, width):
    """d spike / d x, the forms of oracle.snn.surrogate, in the dtype of x."""
    if kind == "arctanspike":
        return 1 / (1 + width * x * x)
    if kind == "superspike":
        return 1 / (1 + width * x.abs()) ** 2
    if kind == "trianglespike":
        return torch.relu(1 - width * x.abs())
    if kind == "mgspike":
        return 1.15 * _gauss(x, 0.0, width) - 0.15 * _gauss(x, width, 6 * width) - 0.15 * _gauss(x, -width, 6 * width)
    raise AttributeError(kind)


def surrogate_scale(kind, x, width):
    """The surrogate with sums of absolute values (numpy fp64).  A Gaussian exp(-a) carries its argument's rounding, a relative
    error of a roundings: its scale is (1 + a) exp(-a)."""
    ax = np.abs(x)
    if kind == "arctanspike":
        return 1 / (1 + width * x * x)
    if kind == "superspike":
        return 1 / (1 + width * ax) ** 2
    if kind == "trianglespike":
        return np.where(1 - width * ax > -1e-3, 1 + width * ax, 0.0)  # (1e-3: either side of the kink within rounding)

    def g(mu, sigma):
        a = (x - mu) * (x - mu) / (2 * sigma * sigma)
        return (1 + a) * np.exp(-a) / (sigma * np.sqrt(2 * np.pi))

    return 1.15 * g(0.0, width) + 0.15 * g(width, 6 * width) + 0.15 * g(-width, 6 * width)


def _surrogate32(kind, x, width):
    """ng_surrogate of the kernels in fp32, operation by operation."""
    w, one = F32(width), F32(1)
    if kind == "superspike":
        d = one + w * np.abs(x)
        return one / (d * d)
    if kind == "trianglespike":
        return np.maximum(F32(0), one - w * np.abs(x))
    if kind == "mgspike":
        k = F32(0.3989422804014327)

        def gs(mu, sg):
            return np.exp(-((x - mu) * (x - mu)) / (F32(2) * sg * sg), dtype=F32) / sg * k

        s2 = F32(6) * w
        return F32(1.15) * gs(F32(0), w) - F32(0.15) * gs(w, s2) - F32(0.15) * gs(-w, s2)
    return one / (one + w * x * x)


class _Spike(torch.autograd.Function):
    """oracle.snn._Spike without the cast to fp32."""

    @staticmethod
    def forward(ctx, x, width, kind):
        ctx.save_for_backward(x)
        ctx.width, ctx.kind = width, kind
        return x.gt(0).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * surrogate_ref(ctx.kind, x, ctx.width), None, None


# -------------------------------------------------------------------------------------------------------------- reference
def _t(a, dtype, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(dtype)  # (a copy: the shared inputs are read-only)
    return t.requires_grad_(True) if grad else t


def _forward_torch(kind, cur, v, z, ax, P, prm, hard, surrogate, width):
    """The four update rules as oracle/snn.py:106-159 states them, on a precomputed cur and P.  -> v_out, z_out, aux_out, th."""
    lam = torch.sigmoid(prm[0])
    a1 = prm[1].clamp_min(CLAMP1)
    zr = z.detach()
    aux_out = None
    th = soft_th = a1
    c = cur
    if kind == "plif":
        leak_pt, add_pt = torch.sigmoid(prm[2]), torch.sigmoid(prm[3])
        aux_out = ax * leak_pt + (1 - leak_pt) * P[:, None]
        c = cur - add_pt * aux_out
    elif kind in ("alif", "xlif"):
        t1, leak_t = prm[2].clamp_min(0), torch.sigmoid(prm[3])
        drive = z if kind == "alif" else P[:, None]  # ALIF's trace reads z NOT detached
        aux_out = ax * leak_t + (1 - leak_t) * drive
        th = a1 + t1 * aux_out
        soft_th = a1 + t1 * ax  # the soft reset reads the OLD trace
    if hard:
        v_out = v * lam * (1 - zr) + (1 - lam) * c
    else:
        v_out = v * lam + (1 - lam) * c - zr * soft_th
    z_out = _Spike.apply(v_out - th, float(F32(width)), surrogate)
    return v_out, z_out, aux_out, th


def neuron_ref(kind, cur, v_prev, z_prev, aux_prev, P, residual, params, hard, surrogate, width, upstream=None,
               dtype=torch.float64):
    """One neuron update and, with `upstream` = {"g_v_out", "g_z_out", "g_z_out2", "g_aux_out"} (any may be missing / None),
    its gradients by torch autograd, all in `dtype`.  Absent previous state = zeros.
    -> {"v_out", "z_out", "aux_out", "out", "th"} and {"g_cur", "g_v_prev", "g_z_prev" (ALIF), "g_aux_prev", "g_P",
    "g_p0" .. "g_p3"} (numpy arrays of that dtype; None where the kind has no such tensor)."""
    need = upstream is not None
    shape = np.asarray(cur).shape
    zeros = np.zeros(shape)
    cur_t = _t(cur, dtype, need)
    v = _t(v_prev if v_prev is not None else zeros, dtype, need)
    z = _t(z_prev if z_prev is not None else zeros, dtype, need)
    ax = _t(aux_prev if aux_prev is not None else zeros, dtype, need) if kind != "lif" else None
    Pt = _t(P, dtype, need) if kind in ("plif", "xlif") else None
    prm = [_t(p, dtype, need) if p is not None else None for p in params]
    v_out, z_out, aux_out, th = _forward_torch(kind, cur_t, v, z, ax, Pt, prm, hard, surrogate, width)
    out = z_out + (_t(residual, dtype) if residual is not None else 0)
    n = lambda t: None if t is None else t.detach().numpy()  # noqa: E731
    res = {"v_out": n(v_out), "z_out": n(z_out), "aux_out": n(aux_out), "out": n(out), "th": n(th + 0 * v_out)}
    if not need:
        return res
    up = {k: _t(upstream.get(k), dtype) for k in ("g_v_out", "g_z_out", "g_z_out2", "g_aux_out")}
    loss = 0
    if up["g_v_out"] is not None:
        loss = loss + (up["g_v_out"] * v_out).sum()
    for k in ("g_z_out", "g_z_out2"):
        if up[k] is not None:
            loss = loss + (up[k] * z_out).sum()
    if up["g_aux_out"] is not None and aux_out is not None:
        loss = loss + (up["g_aux_out"] * aux_out).sum()
    names = ["g_cur", "g_v_prev", "g_z_prev", "g_aux_prev", "g_P", "g_p0", "g_p1", "g_p2", "g_p3"]
    wrt = [cur_t, v, z, ax, Pt] + prm
    have = [(nm, t) for nm, t in zip(names, wrt) if t is not None]
    grads = torch.autograd.grad(loss, [t for _, t in have], allow_unused=True)
    for (nm, t), g in zip(have, grads):
        res[nm] = np.zeros(tuple(t.shape), n(t).dtype) if g is None else n(g)
    for nm in names:
        res.setdefault(nm, None)
    if kind != "alif":
        res["g_z_prev"] = None  # (z is detached in the reset: only ALIF's trace hands z a gradient here)
    return res


def recover_cur64(kind, v_out, aux_out, v_prev, z_prev, aux_prev, params, hard):
    """The current for which the update rule yields exactly `v_out` (fp64): what the backward kernels recover.  aux_out: the
    fp64 trace (PLIF subtracts add_pt * trace from the current)."""
    f = lambda a: np.zeros(np.asarray(v_out).shape) if a is None else np.asarray(a, F64)  # noqa: E731
    vo, v, z, ax = f(v_out), f(v_prev), f(z_prev), f(aux_prev)
    sig = lambda p: 1 / (1 + np.exp(-np.asarray(p, F64)))  # noqa: E731
    lam = sig(params[0])
    a1 = np.maximum(np.asarray(params[1], F64), CLAMP1)
    if hard:
        c = (vo - v * lam * (1 - z)) / (1 - lam)
    else:
        soft_th = a1 + (np.maximum(np.asarray(params[2], F64), 0) * ax if kind in ("alif", "xlif") else 0)
        c = (vo - v * lam + z * soft_th) / (1 - lam)
    if kind == "plif":
        c = c + sig(params[3]) * np.asarray(aux_out, F64)
    return c


def neuron_scales(kind, v_out, aux_out, v_prev, z_prev, aux_prev, P, params, hard, surrogate, width, upstream):
    """The scale beside every gradient output of neuron_ref (numpy fp64): the kernels' expression of that output with absolute
    values throughout (1 - x counts as 1 + |x|; a quotient keeps its denominator)."""
    f = lambda a: np.zeros(np.asarray(v_out).shape) if a is None else np.abs(np.asarray(a, F64))  # noqa: E731
    vo = np.asarray(v_out, F64)
    v, z, ax = f(v_prev), f(z_prev), f(aux_prev)
    ao = f(aux_out) if kind != "lif" else 0.0
    Pv = np.abs(np.asarray(P, F64))[:, None] if kind in ("plif", "xlif") else 0.0
    sig = lambda p: 1 / (1 + np.exp(-np.asarray(p, F64)))  # noqa: E731
    lam = sig(params[0])
    oml = 1 - lam
    a1 = np.maximum(np.asarray(params[1], F64), CLAMP1)
    m1 = (np.asarray(params[1], F64) >= CLAMP1).astype(F64)
    gvo, gza, gzb, ga = (f(upstream.get(k)) for k in ("g_v_out", "g_z_out", "g_z_out2", "g_aux_out"))
    if kind in ("alif", "xlif"):
        a2, a3 = np.maximum(np.asarray(params[2], F64), 0), sig(params[3])
        m2 = (np.asarray(params[2], F64) >= 0).astype(F64)
        th_signed = a1 + a2 * np.asarray(aux_out, F64)
        soft_th = a1 + a2 * ax
    else:
        th_signed = a1 + 0 * vo
        soft_th = a1 + 0 * vo
    if kind == "plif":
        a2, a3 = sig(params[2]), sig(params[3])
    sg = surrogate_scale(surrogate, vo - th_signed, float(F32(width)))
    gsp = (gza + gzb) * sg
    G = gvo + gsp
    gth = gsp
    avo = np.abs(vo)
    if hard:
        gp = G * lam * (1 + z)
        cT = (avo + v * lam * (1 + z)) / oml
        dlam = v * (1 + z) + cT
        gsoft = 0 * G
    else:
        gp = G * lam
        cT = (avo + v * lam + z * soft_th) / oml
        dlam = v + cT
        gsoft = z * G
    gcT = G * (1 + lam)
    s = {"g_cur": gcT, "g_v_prev": gp, "g_z_prev": None, "g_aux_prev": None, "g_P": None, "g_p2": None, "g_p3": None}
    s["g_p0"] = (G * dlam).sum(0) * lam * (1 + lam)
    s["g_p1"] = (gth + gsoft).sum(0) * m1
    if kind == "plif":
        gpt = ga + a3 * gcT
        s["g_aux_prev"] = gpt * a2
        s["g_P"] = (gpt * (1 + a2)).sum(1)
        s["g_p2"] = (gpt * (ax + Pv)).sum(0) * a2 * (1 + a2)
        s["g_p3"] = (gcT * ao).sum(0) * a3 * (1 + a3)
    elif kind in ("alif", "xlif"):
        gtr = ga + gth * a2
        s["g_aux_prev"] = gtr * a3 + gsoft * a2
        drive = z if kind == "alif" else Pv
        if kind == "alif":
            s["g_z_prev"] = gtr * (1 + a3)
        else:
            s["g_P"] = (gtr * (1 + a3)).sum(1)
        s["g_p2"] = (gth * ao + gsoft * ax).sum(0) * m2
        s["g_p3"] = (gtr * (ax + drive)).sum(0) * a3 * (1 + a3)
    return s


def forward_scales(kind, cur, v_prev, z_prev, aux_prev, P, params, hard):
    """Scales of v_out and aux_out (numpy fp64)."""
    f = lambda a: np.zeros(np.asarray(cur).shape) if a is None else np.abs(np.asarray(a, F64))  # noqa: E731
    c, v, z, ax = f(cur), f(v_prev), f(z_prev), f(aux_prev)
    sig = lambda p: 1 / (1 + np.exp(-np.asarray(p, F64)))  # noqa: E731
    lam = sig(params[0])
    a1 = np.maximum(np.asarray(params[1], F64), CLAMP1)
    soft_th = a1 + 0 * c
    aux = None
    if kind != "lif":
        lk = sig(params[2] if kind == "plif" else params[3])
        drive = z if kind == "alif" else np.abs(np.asarray(P, F64))[:, None]
        aux = ax * lk + (1 + lk) * drive
        if kind == "plif":
            c = c + sig(params[3]) * aux
        else:
            soft_th = a1 + np.maximum(np.asarray(params[2], F64), 0) * ax
    vs = v * lam * (1 + z) + (1 + lam) * c if hard else v * lam + (1 + lam) * c + z * soft_th
    return {"v_out": vs, "aux_out": aux}


# -------------------------------------------------------------------------------------------------------------- emulation
def _sig32(x):
    return F32(1) / (F32(1) + np.exp(-np.asarray(x, F32), dtype=F32))


def _z32(a, shape):
    return np.zeros(shape, F32) if a is None else np.asarray(a, F32)


def emulate32_fwd(kind, cur, v_prev, z_prev, aux_prev, P, residual, params, hard, mutant=None):
    """k_neuron_fwd in fp32, operation by operation (the library is built without FMA contraction)."""
    cur = np.asarray(cur, F32)
    one = F32(1)
    v, z, ax = (_z32(a, cur.shape) for a in (v_prev, z_prev, aux_prev))
    lam = _sig32(params[0])
    a1 = np.maximum(np.asarray(params[1], F32), F32(0.01))
    th = soft_th = a1 + 0 * cur
    c, ao = cur, None
    if kind == "plif":
        a2, a3 = _sig32(params[2]), _sig32(params[3])
        ao = ax * a2 + (one - a2) * np.asarray(P, F32)[:, None]
        c = cur - a3 * ao
    elif kind in ("alif", "xlif"):
        a2, a3 = np.maximum(np.asarray(params[2], F32), F32(0)), _sig32(params[3])
        ao = ax * a3 + (one - a3) * (z if kind == "alif" else np.asarray(P, F32)[:, None])
        th = a1 + a2 * ao
        soft_th = a1 + a2 * (ao if mutant == "soft_reset_new_trace" else ax)
    if hard:
        vo = v * lam * (one - z) + (one - lam) * c
    else:
        vo = v * lam + (one - lam) * c - z * soft_th
    zo = ((vo - th) > 0).astype(F32)
    out = zo + (np.asarray(residual, F32) if residual is not None else F32(0))
    assert vo.dtype == F32 and out.dtype == F32
    return {"v_out": vo, "z_out": zo, "aux_out": ao, "out": out}


def emulate32_bwd(kind, v_out, aux_out, v_prev, z_prev, aux_prev, P, params, hard, surrogate, width, upstream, mutant=None):
    """k_neuron_bwd in fp32 in the kernel's operation order: cur recovered from v_out, the clamp masks, the lam (1 - lam) factors
    applied after the sums.  The sums over pixels / channels run in index order.  mutant: one of MUTANTS, a deliberately wrong
    variant."""
    assert mutant is None or mutant in MUTANTS, mutant
    vo = np.asarray(v_out, F32)
    one = F32(1)
    v, z, ax = (_z32(a, vo.shape) for a in (v_prev, z_prev, aux_prev))
    gvo, gza, gzb, ga = (_z32(upstream.get(k), vo.shape) for k in ("g_v_out", "g_z_out", "g_z_out2", "g_aux_out"))
    ao = np.asarray(aux_out, F32) if kind != "lif" else None
    Pv = np.asarray(P, F32)[:, None] if kind in ("plif", "xlif") else None
    p1 = np.asarray(params[1], F32)
    lam = _sig32(params[0])
    a1 = np.maximum(p1, F32(0.01))
    m1 = ((p1 > F32(0.01)) if mutant == "clamp_mask_gt" else (p1 >= F32(0.01))).astype(F32)
    th = soft_th = a1 + 0 * vo
    if kind == "plif":
        a2, a3 = _sig32(params[2]), _sig32(params[3])
    elif kind != "lif":
        p2 = np.asarray(params[2], F32)
        a2, a3 = np.maximum(p2, F32(0)), _sig32(params[3])
        m2 = ((p2 > 0) if mutant == "clamp_mask_gt" else (p2 >= 0)).astype(F32)
        th = a1 + a2 * ao
        soft_th = a1 + a2 * (ao if mutant == "soft_reset_new_trace" else ax)
    oml = one - lam
    sg = _surrogate32(surrogate, vo - th, width)
    gz = gza if mutant == "g_z_out2_ignored" else gza + gzb
    gsp = gz * sg
    G = gvo + gsp
    gth = -gsp
    if hard:
        gp = G * lam * (one - z)
        cT = (vo - (v * lam) * (one - z)) / oml
        dlam = v * (one - z) - cT
        gsoft = np.zeros_like(G)
    else:
        gp = G * lam
        cT = (vo - v * lam + z * soft_th) / oml
        dlam = v - cT
        gsoft = -z * G
    gcT = G * oml
    r = dict.fromkeys(("g_z_prev", "g_aux_prev", "g_P", "g_p2", "g_p3"))
    r["g_cur"], r["g_v_prev"] = gcT, gp
    last = -1 if mutant == "last_pixel_dropped" else None
    S = lambda a: np.add.reduce(a[:last], axis=0, dtype=F32)  # noqa: E731
    r["g_p0"] = S(G * dlam) * lam * (one - lam)
    r["g_p1"] = S(gth + gsoft) * m1
    if kind == "plif":
        gpt = ga - a3 * gcT
        r["g_aux_prev"] = gpt * a2
        r["g_P"] = np.add.reduce(gpt if mutant == "g_P_without_one_minus_leak" else gpt * (one - a2), axis=1, dtype=F32)
        r["g_p2"] = S(gpt * (ax - Pv)) * a2 * (one - a2)
        r["g_p3"] = S(-(gcT * ao)) * a3 * (one - a3)
    elif kind != "lif":
        gtr = ga + gth * a2
        if mutant == "soft_reset_new_trace":
            gtr = gtr + gsoft * a2  # (the soft threshold then hangs on the new trace)
            r["g_aux_prev"] = gtr * a3
        else:
            r["g_aux_prev"] = gtr * a3 + gsoft * a2
        if kind == "alif":
            gzp = gtr * (one - a3)
            if mutant == "z_not_detached":
                gzp = gzp - (G * (v * lam) if hard else G * soft_th)
            if mutant == "alif_g_z_prev_dropped":
                gzp = np.zeros_like(gzp)
            r["g_z_prev"] = gzp
        else:
            r["g_P"] = np.add.reduce(gtr if mutant == "g_P_without_one_minus_leak" else gtr * (one - a3), axis=1, dtype=F32)
        soft_on = ao if mutant == "soft_reset_new_trace" else ax
        r["g_p2"] = S(gth * ao if mutant == "t1_without_gsoft_term" else gth * ao + gsoft * soft_on) * m2
        r["g_p3"] = S(gtr * (ax - (z if kind == "alif" else Pv))) * a3 * (one - a3)
    for k, a in r.items():
        assert a is None or a.dtype == F32, k
    return r


def mutant_applies(mutant, kind, hard, gst, prev):
    """Whether the mistake changes anything a test can see in this configuration."""
    soft_trace = kind in ("alif", "xlif") and not hard and prev != "absent"
    return {
        "clamp_mask_gt": True,
        "soft_reset_new_trace": soft_trace,
        "z_not_detached": kind == "alif" and prev == "present",
        "alif_g_z_prev_dropped": kind == "alif" and prev == "present",
        "g_P_without_one_minus_leak": kind in ("plif", "xlif"),
        "g_z_out2_ignored": gst,
        "t1_without_gsoft_term": soft_trace,
        "last_pixel_dropped": True,
    }[mutant]


# ------------------------------------------------------------------------------------------------------------------ cases
def _seed(*key):
    import zlib

    return zlib.crc32(repr(key).encode())


def make_case(kind, C, npix, hard, gst=True, prev="present", real_z=False):
    """_make_case, cached: every small case for the whole session, the two latest large ones."""
    f = _make_small if C * npix <= 1 << 16 else _make_large
    return f(kind, C, npix, hard, gst, prev, real_z)


def _make_case(kind, C, npix, hard, gst, prev, real_z):
    """Inputs of one case, generated once per key and shared read-only: |cur|, |v| <= 8; spikes in {0, 1} at a rate near 0.3
    (real_z: normally distributed, what a group-norm cell hands to the reset); leak logits in [-4, 4]; thresh / t0 in
    {0.005, 0.01, 0.3} and t1 in {-0.1, 0, 0.2} -- channels below, exactly at and above each clamp; cur nudged until no fp64 v_out
    lies within MARGIN = 1e-4 of its threshold (over 100 fp32 roundings of the largest operand, 8 * 2^-24 = 4.8e-7, where the update
    makes fewer than ten): spikes are compared exactly and no element is excluded.
    -> dict: cur, v_prev, z_prev, aux_prev (None when prev == "absent"), P, residual, params [4], upstream {..}, surrogate,
    width, ref_fwd (neuron_ref in fp64)."""
    rng = np.random.default_rng(_seed(kind, C, npix, hard, gst, prev, real_z))
    shape = (npix, C)
    u = lambda lo, hi, sh=shape: rng.uniform(lo, hi, sh).astype(F32)  # noqa: E731
    d = {"kind": kind, "C": C, "npix": npix, "hard": hard, "gst": gst, "prev": prev}
    d["cur"] = u(-8, 8)
    has_prev = prev != "absent"
    d["v_prev"] = u(-8, 8) if has_prev else None
    if has_prev:
        d["z_prev"] = rng.normal(0, 1, shape).astype(F32) if real_z else (rng.random(shape) < 0.3).astype(F32)
    else:
        d["z_prev"] = None
    d["aux_prev"] = u(0, 1.5) if (has_prev and kind != "lif") else None
    d["P"] = u(0, 2, (npix,)) if kind in ("plif", "xlif") else None
    d["residual"] = rng.integers(0, 3, shape).astype(F32)
    cyc = lambda vals: np.asarray(vals, F32)[(np.arange(C) + int(rng.integers(0, 3))) % 3]  # noqa: E731
    p0, p1 = u(-4, 4, (C,)), cyc([0.005, 0.01, 0.3])
    if kind == "lif":
        prm = [p0, p1, None, None]
    elif kind == "plif":
        prm = [p0, p1, u(-4, 4, (C,)), u(-4, 4, (C,))]
    else:
        prm = [p0, p1, np.asarray([-0.1, 0.0, 0.2], F32)[(np.arange(C) // 3 + np.arange(C)) % 3], u(-4, 4, (C,))]
    d["params"] = prm
    g = lambda sh=shape: rng.normal(0, 1, sh).astype(F32)  # noqa: E731
    d["upstream"] = {"g_z_out": g(), "g_v_out": g() if gst else None, "g_z_out2": g() if gst else None,
                     "g_aux_out": g() if (gst and kind != "lif") else None}
    d["surrogate"] = SURROGATES[_seed(kind, C, npix, hard, gst, prev) % 4]
    d["width"] = WIDTH[d["surrogate"]]
    oml = 1 - 1 / (1 + np.exp(-p0.astype(F64)))
    for _ in range(8):
        ref = neuron_ref(kind, d["cur"], d["v_prev"], d["z_prev"], d["aux_prev"], d["P"], d["residual"], prm, hard,
                         d["surrogate"], d["width"])
        x = ref["v_out"] - ref["th"]
        close = np.abs(x) < 2 * MARGIN
        if not close.any():
            break
        step = np.where(x >= 0, 1.0, -1.0) * 8 * MARGIN / oml
        d["cur"] = np.where(close, d["cur"].astype(F64) + step, d["cur"]).astype(F32)
    assert np.abs(ref["v_out"] - ref["th"]).min() > MARGIN, "a membrane potential within the margin of its threshold"
    d["ref_fwd"] = ref
    for a in [d["cur"], d["v_prev"], d["z_prev"], d["aux_prev"], d["P"], d["residual"]] + prm + list(d["upstream"].values()):
        if a is not None:
            a.setflags(write=False)
    return d


_make_small = functools.lru_cache(maxsize=None)(_make_case)
_make_large = functools.lru_cache(maxsize=2)(_make_case)


def backward_reference(case, v_out32, aux_out32):
    """The fp64 gradients of the update that produced the SAVED v_out (teacher forcing: the current is the one that yields
    v_out32 exactly) and their scales.  -> (neuron_ref result, scales)."""
    k, prm, hard = case["kind"], case["params"], case["hard"]
    aux64 = case["ref_fwd"]["aux_out"]
    cur = recover_cur64(k, v_out32, aux64, case["v_prev"], case["z_prev"], case["aux_prev"], prm, hard)
    ref = neuron_ref(k, cur, case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], None, prm, hard, case["surrogate"],
                     case["width"], upstream=case["upstream"])
    sc = neuron_scales(k, v_out32, aux_out32, case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], prm, hard,
                       case["surrogate"], case["width"], case["upstream"])
    return ref, sc


def units(got, ref, scale):
    """max |got - ref| / (2^-24 scale); elements of scale 0 must agree exactly (inf otherwise)."""
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64)).reshape(-1)
    sc = U * np.asarray(scale, F64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(sc > 0, err / sc, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------------------------------------------------- launch geometry
def bwd_geometry(C, npix):
    """Block size, blocks, trips and the reduction arm of evf_neuron_bwd, from the header comment of its host wrapper: a block
    holds (256 / Q) * Q threads (256 from Q = 256 on); one float4 per thread and at most 64 blocks until a block would see four
    float4 per thread, then total / (4 * block) blocks, 1024 at the most; more than 256 blocks go through 32 replicas."""
    Q = C // 4
    bs = 256 if Q >= 256 else (256 // Q) * Q
    total = npix * Q
    want = -(-total // (bs * 4))
    if want < 64:
        want = min(-(-total // bs), 64)
    nblk = min(want, 1024)
    trips = -(-total // (nblk * bs))
    np2 = Q < 64 and (Q & (Q - 1)) != 0
    return {"Q": Q, "bs": bs, "nblk": nblk, "trips": trips, "np2": np2, "replicas": nblk > 256}


def chain_terms(C, npix, ws=True):
    """Additions a term of a parameter sum can pass through in an unknown order, in units of 2^-24 * scale:
    trips + shuffle levels + adds into the block's LDS word + adds per output address (+ 1 onto the initial contents).
    -> (parameter sums, g_P)."""
    g = bwd_geometry(C, npix)
    Q, bs = g["Q"], g["bs"]
    pow2_small = Q < 64 and not g["np2"]
    shuffles = int(np.log2(64 // Q)) if pow2_small else 0
    lds = -(-bs // 64) if pow2_small else bs // Q
    if g["replicas"] and ws:
        per_address = -(-g["nblk"] // 32) + 32
    else:
        per_address = g["nblk"]
    gp = 4 + (int(np.ceil(np.log2(Q))) if (Q <= 64 and not g["np2"]) else Q)
    return g["trips"] + shuffles + lds + per_address + 1, gp


# ------------------------------------------------------------------------------------------------------------------ leaky
ACTS = (None, "tanh", "sigmoid", "relu")  # evf_act ids 0..3
# Bound of the leaky kernels, by reasoning (units of 2^-24 * scale): lam = 1 / (1 + exp(-x)) carries the exp (2 ulp of a device
# libm), an add and a divide, <= 4 roundings; 1 - lam one more; each product and sum one: mix = prev lam + (1 - lam)(cur + res)
# stays below 8 units of |prev| lam + (1 + lam)(|cur| + |res|), the activation (<= 2 ulp of its own value, plus its slope times
# the error of mix) below 8 more.  K_LEAKY = 16.  In the backward the recovered current (mix - prev lam) / (1 - lam) divides by
# 1 - lam, whose RELATIVE error is up to 5 lam / (1 - lam) roundings: the scale of that quotient carries the factor
# (1 + lam / (1 - lam)).
K_LEAKY = 16.0


def _act(name, x):
    return x if name is None else getattr(torch, name)(x)


def leaky_ref(cur, prev, residual, leak, act, g_out=None, g_state=None, dtype=torch.float64):
    """ConvLeaky / ConvLeakyRecurrent algebra (oracle.snn.conv_leaky_step): mix = prev lam + (1 - lam)(cur + residual),
    out = act(mix); gradients of sum(g_out out) + sum(g_state mix) by autograd.  -> dict of numpy arrays incl. the scales
    "s_mix", "s_out", "s_g_cur", "s_g_prev", "s_g_leak"."""
    need = g_out is not None or g_state is not None
    shape = np.asarray(cur).shape
    c = _t(cur, dtype, need)
    p = _t(prev if prev is not None else np.zeros(shape), dtype, need)
    lk = _t(leak, dtype, need)
    lam = torch.sigmoid(lk)
    r = _t(residual, dtype) if residual is not None else 0
    mix = p * lam + (1 - lam) * (c + r)
    out = _act(act, mix)
    n = lambda t: t.detach().numpy()  # noqa: E731
    res = {"mix": n(mix), "out": n(out)}
    f = lambda a: np.zeros(shape) if a is None else np.abs(np.asarray(a, F64))  # noqa: E731
    lam64 = 1 / (1 + np.exp(-np.asarray(leak, F64)))
    res["s_mix"] = f(prev) * lam64 + (1 + lam64) * (f(cur) + f(residual))
    o = np.abs(res["out"])
    slope = {None: 1.0, "tanh": 1 + o * o, "sigmoid": o * (1 + o), "relu": 1.0}[act]
    res["s_out"] = o + slope * res["s_mix"]
    if not need:
        return res
    loss = 0
    if g_out is not None:
        loss = loss + (_t(g_out, dtype) * out).sum()
    if g_state is not None:
        loss = loss + (_t(g_state, dtype) * mix).sum()
    gc, gp, gl = torch.autograd.grad(loss, [c, p, lk], allow_unused=True)
    res.update(g_cur=n(gc), g_prev=n(gp), g_leak=n(gl))
    G = f(g_state) + f(g_out) * slope
    oml = 1 - lam64
    cT = (np.abs(np.asarray(res["mix"], F64)) + f(prev) * lam64) / oml * (1 + lam64 / oml)
    res.update(s_g_cur=G * (1 + lam64), s_g_prev=G * lam64, s_g_leak=(G * (f(prev) + cT)).sum(0) * lam64 * (1 + lam64))
    return res


# --------------------------------------------------------------------------------------------------------------- pretrace
def pretrace_ref(x_nhwc, k, stride, g_P=None, dtype=torch.float64):
    """P = F.avg_pool2d(x.abs().mean(1), k, stride, k // 2) on an NHWC input [B][H][W][C] and, with g_P [B][Ho][Wo], its autograd.
    -> {"P", "g_x" (NHWC), "s_g_x": pool^T(|g_P|) / C (NHWC scale)}."""
    x = _t(x_nhwc, dtype, g_P is not None)
    m = x.abs().mean(3, keepdim=False)[:, None]
    P = torch.nn.functional.avg_pool2d(m, k, stride, padding=k // 2)[:, 0]
    res = {"P": P.detach().numpy()}
    if g_P is not None:
        (gx,) = torch.autograd.grad((P * _t(g_P, dtype)).sum(), [x])
        res["g_x"] = gx.detach().numpy()
        ones = torch.ones(x.shape, dtype=dtype, requires_grad=True)
        Pa = torch.nn.functional.avg_pool2d(ones.mean(3)[:, None], k, stride, padding=k // 2)[:, 0]
        (sx,) = torch.autograd.grad((Pa * _t(np.abs(g_P), dtype)).sum(), [ones])
        res["s_g_x"] = sx.detach().numpy()
    return res
