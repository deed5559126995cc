"""References of the evaluation-metric kernels of evf_events.hip (evf_image_variance, evf_avg_ts_ratio, evf_aee, evf_mask_union,
evf_masked_flow_mean, evf_apply_pixel_mask) and of evf_norm_nonzero / evf_norm_nonzero_det, shared by
tests/test_host_metrics_reference.py (CPU) and tests/test_gpu_metrics.py.  Not a test module.

The scheme of tests/zoo_ops_ref.py (whose Out / fractions / rules 1 - 3 are used as they stand): CASES[family], make(family, case),
run(family, case, inputs, dtype, mut) -- float64 the reference, float32 the emulation with the kernels' association (a block of
1024 threads: a strided loop per thread, the xor butterfly of every wave, the butterfly over the waves' sums), `mut` one of
MUTANTS -- and expect(family, case, inputs).  Rule 4 on top: the counts of evf_aee (valid pixels, outliers) are asserted exactly;
aee_margins() states by how much every comparison of the float64 reference clears its threshold (the host test asserts 1e-3
relative on every pixel), and the count of evf_avg_ts_ratio is decided by integer-valued event counts."""

import functools

import numpy as np

import zoo_ops_ref as Z
from zoo_ops_ref import F32, F64, Out, U, fractions  # noqa: F401  (re-exported)

MUTANTS = ("var_div_hw", "var_one_pass", "aee_or", "aee_ratio_of_sample_0", "union_without_min", "mean_without_eps")
MEASURED = {"variance.real": 163, "ts_ratio": 1.7, "aee.se": 0.846, "masked_mean.real": 3.13, "norm_nonzero": 2.55}
K2 = {"mask_union.real": lambda P: P}  # the P additions of the sum (min is exact)

HWS = (2, 63, 64, 1023, 1024, 1025, 5 * 7, 260 * 346)
FLOW_SCALING = 32.0


def block_sum(v, threads=1024):
    """evf_block_sum over the last axis in v's dtype: thread t adds elements t, t + threads, ... in order; the xor butterfly
    inside every wave of 64; the butterfly over the (zero-padded) wave sums."""
    lead, n = v.shape[:-1], v.shape[-1]
    trips = Z.cdiv(n, threads)
    t = np.zeros(lead + (trips * threads,), v.dtype)
    t[..., :n] = v
    t = t.reshape(lead + (trips, threads))
    acc = np.zeros(lead + (threads,), v.dtype)
    for j in range(trips):
        acc = acc + t[..., j, :]
    lane = np.arange(64)

    def butterfly(w):
        o = 32
        while o:
            w = w + w[..., lane ^ o]
            o >>= 1
        return w[..., 0]

    waves = butterfly(acc.reshape(lead + (threads // 64, 64)))
    pad = np.zeros(lead + (64,), v.dtype)
    pad[..., :threads // 64] = waves
    return butterfly(pad)


# ================================================================================================================== variance
VAR_CASES = [(kind, B, HW) for kind in ("exact", "real") for B in (1, 3) for HW in HWS]


def _make_variance(case):
    """exact: integer pixels whose sum is a multiple of HW (mean and deviations are integers, every partial sum far below 2^24).
    real: mean 1e3, sigma 1 -- the one-pass form E x^2 - (E x)^2 loses every digit of it in float32."""
    kind, B, HW = case
    rng = Z._rng(101, B, HW)
    if kind == "real":
        return {"img": rng.normal(1e3, 1.0, (B, HW)).astype(F32)}
    img = rng.integers(-3, 4, (B, HW)).astype(np.int64)
    for b in range(B):
        img[b, :int(img[b].sum() % HW)] -= 1
    img += 5 + np.arange(B)[:, None]
    assert not (img.sum(1) % HW).any()
    return {"img": img.astype(F32)}


def _run_variance(case, i, dt, mut):
    kind, B, HW = case
    im = Z._c(i["img"], dt)
    n = dt(HW)
    if mut == "var_one_pass":
        s, q = block_sum(im), block_sum(im * im)
        v = q - s * s / n
    else:
        mean = block_sum(im) / n
        d = im - mean[:, None]
        v = block_sum(d * d)
    return {"var": v / (n if mut == "var_div_hw" else dt(HW - 1))}


# ================================================================================================================== ts ratio
TS_CASES = [(P, HW) for P in (1, 10) for HW in HWS]


def _make_ts(case):
    """images [3, 4, HW]: event counts per polarity (integers 0 .. 3, about half of the pixels without any event), summed
    timestamps; at every 5th event-free pixel a timestamp residue of 2e-9 (in the sum of squares, not in the count).  Sample 2
    has no events at all: 0 / 0."""
    P, HW = case
    rng = Z._rng(103, HW)
    cnt = rng.integers(0, 4, (3, 2, HW)) * (rng.random((3, 1, HW)) < 0.5)
    ts = cnt * rng.uniform(0.0, float(P), (3, 2, HW))
    empty = cnt.sum(1, keepdims=True) == 0
    ts = np.where(empty & (np.arange(HW) % 5 == 0), 2e-9, ts)
    im = np.concatenate([cnt, ts], 1).astype(F32)
    im[2] = 0.0
    return {"images": im}


def _run_ts(case, i, dt, mut):
    P, HW = case
    im = Z._c(i["images"], dt)
    ip, in_, tp, tn = im[:, 0], im[:, 1], im[:, 2], im[:, 3]
    eps, Pd = dt(F32(1e-9)), dt(P)
    ap, an = tp / (ip + eps) / Pd, tn / (in_ + eps) / Pd
    sq = block_sum(ap * ap + an * an)
    nz = block_sum(((ip + in_) > 0).astype(dt))
    with np.errstate(invalid="ignore"):
        return {"out": sq / nz}


# ======================================================================================================================= AEE
AEE_CASES = [(B, H, W) for B in (1, 3) for (H, W) in ((5, 7), (33, 70))]
AEE_RATIO = (0.5, 1.25, 2.0)  # dt_gt / dt_input per sample
AEE_MARGIN = 1e-3


def aee_terms(i, dt, mut=None):
    """Per pixel: (err, mag, valid) of evf_aee in dtype dt (loss/flow.py:594-628)."""
    f, g, m = Z._c(i["flow"], dt), Z._c(i["gt"], dt), Z._c(i["mask"], dt)
    r = Z._c(i["ratio"], dt)
    r = (np.full_like(r, r[0]) if mut == "aee_ratio_of_sample_0" else r)[:, None, None, None]
    S = dt(F32(FLOW_SCALING))
    fl = f * S * r
    valid = (m != 0) & ~((g[:, 0] == 0) & (g[:, 1] == 0))
    dx, dy = fl[:, 0] - g[:, 0], fl[:, 1] - g[:, 1]
    err = np.where(valid, np.sqrt(dx * dx + dy * dy), dt(0))
    mag = np.where(valid, np.sqrt(fl[:, 0] * fl[:, 0] + fl[:, 1] * fl[:, 1]), dt(0))
    return err, mag, valid


def aee_margins(i):
    """Relative distance of every pixel's two comparisons from their thresholds in the float64 reference (inf: decided exactly,
    an invalid pixel's err = 0 against 3 and 0 against 0.05 * 0)."""
    err, mag, valid = aee_terms(i, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(valid, np.abs(err - 3.0) / 3.0, np.inf)
        b = np.where(valid, np.abs(err - 0.05 * mag) / np.maximum(err, 0.05 * mag), np.inf)
    return a, b


def _make_aee(case):
    """flow [B, 2, HW] (network units: times flow_scaling 32 and the sample's ratio gives pixels), gt, mask, ratio.  Every 7th
    pixel a large flow (|f| ~ 100 px) whose ground truth lies about 4 px off: err > 3 but not > 5 % of the magnitude.  The mask
    holds 0 (a third), 1, 0.5, 2 and -1; gt = (0, 0) at every 4th pixel, one zero component at every 9th / 10th.  Pixels whose
    comparisons come within 2e-3 of a threshold are drawn again."""
    B, H, W = case
    HW = H * W
    rng = Z._rng(107, B, H, W)
    ratio = np.asarray(AEE_RATIO[:B], F32) if B > 1 else np.asarray([1.25], F32)
    idx = np.arange(HW)

    def draw():
        flow = rng.normal(0, 0.08, (B, 2, HW))
        gt = flow * FLOW_SCALING * ratio[:, None, None].astype(F64) + rng.normal(0, 2.5, (B, 2, HW))
        big = rng.normal(0, 1, (B, 2, HW))
        big = 100.0 * big / np.sqrt((big ** 2).sum(1, keepdims=True))
        off = rng.normal(0, 1, (B, 2, HW))
        off = rng.uniform(3.3, 4.7, (B, 1, HW)) * off / np.sqrt((off ** 2).sum(1, keepdims=True))
        sel = (idx % 7 == 3)
        gt = np.where(sel, big + off, gt)
        flow = np.where(sel, big / FLOW_SCALING / ratio[:, None, None].astype(F64), flow)
        return flow.astype(F32), gt.astype(F32)

    flow, gt = draw()
    mask = np.asarray([0.0, 1.0, 1.0, 0.5, 0.0, 2.0, 1.0, -1.0, 1.0], F32)[rng.integers(0, 9, (B, HW))]
    for _ in range(20):
        gt2 = gt.copy()
        gt2[:, :, idx % 4 == 1] = 0.0
        gt2[:, 0, idx % 9 == 2] = 0.0
        gt2[:, 1, idx % 10 == 5] = 0.0
        i = {"flow": flow.reshape(B, 2, H, W), "gt": gt2.reshape(B, 2, H, W), "mask": mask.reshape(B, H, W), "ratio": ratio}
        a, b = aee_margins(i)
        close = ((a < 2 * AEE_MARGIN) | (b < 2 * AEE_MARGIN)).reshape(B, 1, HW)
        if not close.any():
            return i
        f2, g2 = draw()
        flow, gt = np.where(close, f2, flow), np.where(close, g2, gt)
    raise AssertionError("no inputs with the margin")


def _run_aee(case, i, dt, mut):
    B = case[0]
    err, mag, valid = aee_terms(i, dt, mut)
    c1, c2 = err > dt(3), err > dt(F32(0.05)) * mag
    outl = (c1 | c2) if mut == "aee_or" else (c1 & c2)
    flat = lambda a: a.reshape(B, -1).astype(dt)  # noqa: E731
    return {"se": block_sum(flat(err)), "nv": block_sum(flat(valid)), "no": block_sum(flat(outl))}


# ==================================================================================================================== masks
MASK_CASES = [(kind, B, P, H, W) for kind in ("exact", "real") for B in (1, 3) for P in (1, 2, 7) for (H, W) in ((5, 7), (13, 23))]


def _make_masks(case):
    """masks [B, P, HW]: binary (exact) or fractional weights (real), every 3rd pixel masked in no pass; maps [B, P, 2, HW]: dyadic
    flows k / 8 with |k| <= 64 (exact: every product and sum is exact) or real."""
    kind, B, P, H, W = case
    HW = H * W
    rng = Z._rng(109, B, P, HW)
    on = rng.random((B, P, HW)) < 0.5
    on[:, :, np.arange(HW) % 3 == 0] = False
    if kind == "exact":
        return {"masks": on.astype(F32), "maps": (rng.integers(-64, 65, (B, P, 2, HW)) / 8.0).astype(F32)}
    return {"masks": (on * rng.uniform(0.1, 0.9, (B, P, HW))).astype(F32), "maps": rng.normal(0, 1, (B, P, 2, HW)).astype(F32)}


def _run_union(case, i, dt, mut):
    m = Z._c(i["masks"], dt)
    s = np.zeros_like(m[:, 0])
    for p in range(case[2]):
        s = s + m[:, p]
    return {"out": s if mut == "union_without_min" else np.minimum(s, dt(1)), "_s": s}


def _run_masked_mean(case, i, dt, mut):
    """The denominator's 1e-9 is the FLOAT32 constant added in the working precision for both dtypes' counts of a binary mask (it
    vanishes against a count >= 1 in float32: the exact case expects the correctly rounded sx / count, and 0 / 1e-9 = 0)."""
    kind, B, P = case[0], case[1], case[2]
    m, f = Z._c(i["masks"], dt), Z._c(i["maps"], dt)
    sx = np.zeros_like(f[:, 0])
    sa = np.zeros_like(f[:, 0])
    sm = np.zeros_like(m[:, 0])
    for p in range(P):
        t = f[:, p] * m[:, p, None]
        sx, sa, sm = sx + t, sa + np.abs(t), sm + m[:, p]
    if mut == "mean_without_eps":
        den = sm
    elif kind == "exact":
        den = (sm.astype(F32) + F32(1e-9)).astype(dt)
    else:
        den = sm + dt(F32(1e-9))
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"out": sx / den[:, None], "_s": sa / den[:, None]}


PIXMASK_CASES = [(1, 1, 15, 17), (1, 1, 16, 16), (1, 1, 1, 257), (1, 2, 8, 16), (3, 5, 1, 17), (1, 5, 7, 11), (2, 2, 5, 13), (3, 2, 16, 16)]


def _make_pixmask(case):
    B, C, H, W = case
    rng = Z._rng(113, *case)
    m = (rng.random((B, H * W)) < 0.8).astype(F32)
    m[:, ::7] = 0.5
    return {"x": rng.normal(0, 1, (B, C, H * W)).astype(F32), "mask": m}


def _run_pixmask(case, i, dt, mut):
    return {"x": Z._c(i["x"], dt) * Z._c(i["mask"], dt)[:, None, :]}


# ============================================================================================================ norm_nonzero
NZ_N = (2, 3, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1)
NZ_CASES = [("half", n) for n in NZ_N] + [(k, n) for k in ("zeros", "one") for n in (2, 3, 1025, 2 ** 20 + 1)]


def _make_nz(case):
    kind, n = case
    rng = Z._rng(127, n)
    if kind == "zeros":
        return {"x": np.zeros(n, F32)}
    if kind == "one":
        x = np.zeros(n, F32)
        x[n // 2] = -1.75
        return {"x": x}
    x = (0.8 * rng.standard_normal(n) + 0.2).astype(F32)
    x[rng.random(n) < 0.5] = 0.0
    x[0], x[-1] = 0.7, -1.3  # (n = 2: two non-zero entries)
    return {"x": x}


def _run_nz(case, i, dt, mut):
    """models/model.py:247-252: x[x != 0] = (x[x != 0] - mean) / std over the non-zero entries, std unbiased.  The kernels sum in
    float64 and round mean and std to float32 before the element pass: so does the float32 emulation."""
    x64 = np.asarray(i["x"], F64)
    nzm = x64 != 0
    c = float(nzm.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(x64[nzm].sum()) / np.float64(c)
        sd = np.sqrt(np.float64(((x64[nzm] - mean) ** 2).sum()) / np.float64(c - 1.0))
        mean, sd = dt(mean), dt(sd)
        x = Z._c(i["x"], dt)
        out = np.where(nzm, (x - mean) / sd, dt(0))
        return {"out": out, "_s": np.where(nzm, (np.abs(x) + abs(mean)) / sd, 1.0)}


# ================================================================================================================== the table
CASES = {"variance": VAR_CASES, "ts_ratio": TS_CASES, "aee": AEE_CASES, "mask_union": MASK_CASES, "masked_mean": MASK_CASES,
         "pixel_mask": PIXMASK_CASES, "norm_nonzero": NZ_CASES}
_MAKE = {"variance": _make_variance, "ts_ratio": _make_ts, "aee": _make_aee, "mask_union": _make_masks, "masked_mean": _make_masks,
         "pixel_mask": _make_pixmask, "norm_nonzero": _make_nz}
_RUN = {"variance": _run_variance, "ts_ratio": _run_ts, "aee": _run_aee, "mask_union": _run_union, "masked_mean": _run_masked_mean,
        "pixel_mask": _run_pixmask, "norm_nonzero": _run_nz}
FAMILIES = tuple(CASES)
MUTANT_FAMILIES = {"var_div_hw": ("variance",), "var_one_pass": ("variance",), "aee_or": ("aee",), "aee_ratio_of_sample_0": ("aee",),
                   "union_without_min": ("mask_union",), "mean_without_eps": ("masked_mean",)}


@functools.lru_cache(maxsize=None)
def make(family, case):
    return Z._freeze(dict(_MAKE[family](case)))


def run(family, case, inputs, dtype=F64, mut=None):
    assert mut is None or mut in MUTANTS, mut
    return _RUN[family](case, inputs, dtype, mut)


def expect(family, case, inputs):
    r = run(family, case, inputs, F64)
    exact = case[0] == "exact"
    if family == "variance":
        return {"var": Out(Z.r32(r["var"]), 1)} if exact else {"var": Out(r["var"], 3, r["var"], key="variance.real", table=MEASURED)}
    if family == "ts_ratio":
        return {"out": Out(r["out"], 3, np.nan_to_num(r["out"]), key="ts_ratio", table=MEASURED)}
    if family == "aee":
        return {"se": Out(r["se"], 3, r["se"], key="aee.se", table=MEASURED), "nv": Out(r["nv"], 1), "no": Out(r["no"], 1)}
    if family == "mask_union":
        return {"out": Out(r["out"], 1)} if exact else {"out": Out(r["out"], 2, r["_s"] + 1e-30, k=K2["mask_union.real"](case[2]))}
    if family == "masked_mean":
        return {"out": Out(Z.r32(r["out"]), 1)} if exact else {"out": Out(r["out"], 3, r["_s"], key="masked_mean.real", table=MEASURED)}
    if family == "pixel_mask":
        return {"x": Out(Z.r32(r["x"]), 1)}
    if case[0] == "half":
        return {"out": Out(r["out"], 3, r["_s"], key="norm_nonzero", table=MEASURED)}
    return {"out": Out(r["out"], 1)}  # zeros: all zeros;  one: NaN at the non-zero element, zeros elsewhere
