"""The float64 reference of evf_aee_at (csrc/evf_eval_log.hip), shared by tests/test_gpu_aee_at.py.  Not a test module.

Inputs are tests/metrics_ref.py's AEE inputs (masked pixels, ground truth that is zero at some pixels, errors on both sides of 3.0
and of 0.05 |flow|, every comparison cleared by 1e-3 relative) with the ratio given as two device doubles per sample.  The
ratio is float32 BY DEFINITION -- (float)dt_gt / (float)dt_input, one IEEE division, what `torch.as_tensor(.., float32)`
and the division in AEE.forward give -- so the reference starts from that float32 value and does everything behind it in
float64.

The bound of the error sum: the kernel adds non-negative float32 terms, so a chain of d additions is off by at most
d 2^-24 relative of the exact sum, and every term (two multiplies, two subtractions, three products and sums, a square root)
by a few 2^-24 of itself, which the issue's 8 covers: (d + 8) 2^-24 of the float64 sum.  d follows from the launch geometry
(include/evflow.h): a stripe of 2048 pixels over 256 threads is 8 additions per thread, two butterflies of 6 (the wave, the
waves' sums), then the S stripes in order."""

import numpy as np

import metrics_ref as M

F32, F64 = np.float32, np.float64
FLOW_SCALING = M.FLOW_SCALING
STRIPE, THREADS = 2048, 256
DT_INPUT = (0.05, 0.043, 0.07)


def stripes(H, W):
    return -(-(H * W) // STRIPE)


def chain(H, W):
    """d: the longest chain of float32 additions behind one sample's error sum."""
    return STRIPE // THREADS + 6 + 6 + stripes(H, W)


def bound(H, W):
    return (chain(H, W) + 8) * 2.0 ** -24


def ratio32(dt_gt, dt_input):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(dt_gt, F64).astype(F32) / np.asarray(dt_input, F64).astype(F32)


def make(B, H, W, broken=None):
    """flow, gt [B,2,H,W], mask [B,H,W] float32, dt_gt, dt_input float64 [B].  `broken`: "inf" -- the LAST sample has dt_input = 0,
    "nan" -- dt_gt = 0 as well."""
    i = dict(M._make_aee((B, H, W)))
    dt_input = np.asarray(DT_INPUT[:B], F64)
    dt_gt = np.asarray(i.pop("ratio"), F64) * dt_input
    if broken:
        dt_input[-1] = 0.0
        if broken == "nan":
            dt_gt[-1] = 0.0
    i["dt_gt"], i["dt_input"] = dt_gt, dt_input
    return i


def sums(i):
    """Per sample (sum err, n valid, n outliers) in float64 from the float32 ratio; margins: how far every comparison of the
    finite samples stays from its threshold."""
    B = i["flow"].shape[0]
    j = {**i, "ratio": ratio32(i["dt_gt"], i["dt_input"])}
    with np.errstate(invalid="ignore", over="ignore"):
        err, mag, valid = M.aee_terms(j, F64)
        outl = (err > 3.0) & (err > F64(F32(0.05)) * mag)
        a, b = M.aee_margins(j)
    flat = lambda x: x.reshape(B, -1)  # noqa: E731
    finite = np.isfinite(j["ratio"])
    margin = min(float(flat(a)[finite].min()), float(flat(b)[finite].min())) if finite.any() else np.inf
    with np.errstate(invalid="ignore"):
        return flat(err).sum(1), flat(valid).sum(1).astype(F64), flat(outl).sum(1).astype(F64), margin


def row(se, nv, no):
    """The 2 (B + 1) floats of the log row from a sample's three sums, in float32 as launch 2 forms them."""
    se, nv, no = (np.asarray(v, F32) for v in (se, nv, no))
    B = len(se)
    total = F32(0)
    for b in range(B):
        total = F32(total + no[b])
    with np.errstate(invalid="ignore", over="ignore"):
        aee = se / (nv + F32(1e-9))
        pct = total / (nv + F32(1e-9))
        sa = sp = F32(0)
        for b in range(B):
            sa, sp = F32(sa + aee[b]), F32(sp + pct[b])
        return np.concatenate([aee, [sa / F32(B)], pct, [sp / F32(B)]]).astype(F32)
