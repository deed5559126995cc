"""Plain references of the general-path convolutions (csrc/evf_conv_b3gen.hip, evf_conv_b3tile.hip, evf_conv_b3n.hip, evf_conv_b3img.hip,
evf_conv_b3small.hip, evf_conv_gen.hip, evf_wgrad_gen.hip, evf_wgrad_b3gen.hip), shared by tests/test_host_conv_reference.py (which
establishes the bounds below on the CPU and shows that they reject wrong kernels) and tests/test_gpu_conv_products.py (which holds the
kernels to them).  Not a test module itself.

Two legs:
  * IMPULSE: the input is zero except for isolated impulses, so every output element is ONE product x * w or nothing at all.  There
    is no accumulation noise: an element is held to K * 2^-24 * |x * w| (K_IMP for the split products on the bf16 matrix cores, K_F32
    = 1 for the single correctly rounded product of the fp32 kernels) and an element without a product to the exact bits of 0, the
    base or the bias.  This is the leg that notices a dropped split term.
  * DENSE: random operands, every element against float64 within K_SUM * 2^-24 * A_e, A_e = sum |x_i| |w_i| the float64 convolution
    of the absolute values (+ |bias| + |base|).  It notices wrong taps, borders and channel tails, NOT a dropped third-order term
    (2^-16 of a product, below the accumulation noise of a few hundred terms): that is the impulse leg's job.

The split emulation follows csrc/evf_split.h (round to nearest even at every step, exact fp32 residuals); a product of two bf16 values
has 16 significant bits, exact in fp32, so a six-term product is six exact terms added in fp32."""

import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # half an ulp of 1.0 in fp32: the relative error bound of one correctly rounded operation

K_F32 = 1  # the fp32 kernels: one correctly rounded product
K_IMP = 10  # split products: 2 x the largest emulated error in units of 2^-24 |x w|, rounded up (test_host_conv_reference.py)
K_IMP_MAX = 16  # above this the bound no longer rejects a dropped third-order term on more than half of the products
K_SUM = 7  # dense leg: 2 x the largest emulated error of the kernels' association in units of 2^-24 A_e, rounded up (same module)

# the six terms of a split product in the order the kernels issue them (smallest first); index 0 = hi, 1 = mid, 2 = lo plane
TERMS6 = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))  # (x plane, w plane)
TERMS3 = ((0, 2), (0, 1), (0, 0))  # x exactly representable in bf16
DROPPABLE = {"x0w1": (0, 1), "x1w0": (1, 0), "x0w2": (0, 2), "x1w1": (1, 1), "x2w0": (2, 0)}


# ------------------------------------------------------------------------------------------------------------ the bf16 split
def bf16_rne(a):
    """fp32 -> the nearest bf16 (ties to even) as fp32; finite inputs."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(F32).reshape(np.shape(a))


def split3(a):
    """evf_split3_pair: a = hi + mid + lo exactly, every plane a bf16."""
    a = np.asarray(a, F32)
    hi = bf16_rne(a)
    r = (a - hi).astype(F32)
    mid = bf16_rne(r)
    lo = bf16_rne((r - mid).astype(F32))
    return hi, mid, lo


def is_bf16(a):
    a = np.asarray(a, F32)
    return bf16_rne(a) == a


def split_product(x, w, terms=TERMS6, drop=None, reverse=False):
    """The kernels' product of ONE x and ONE w (elementwise over arrays): the listed bf16 terms, each exact in fp32, added in fp32
    from 0 in issue order (or reversed).  drop = an (x plane, w plane) pair left out: the mutants."""
    xs, ws = split3(x), split3(w)
    order = [t for t in terms if t != drop]
    if reverse:
        order = order[::-1]
    acc = np.zeros(np.shape(np.asarray(x, F32) * np.asarray(w, F32)), F32)
    for i, j in order:
        acc = (acc + (xs[i] * ws[j]).astype(F32)).astype(F32)
    return acc


def f32_product(x, w):
    """One correctly rounded fp32 product (the fp64 product of two fp32 values is exact)."""
    return (np.asarray(x, F64) * np.asarray(w, F64)).astype(F32)


def units(got, x, w):
    """|got - x w| in units of 2^-24 |x w| (float64)."""
    ref = np.asarray(x, F64) * np.asarray(w, F64)
    return np.abs(np.asarray(got, F64) - ref) / (U * np.abs(ref))


# ------------------------------------------------------------------------------------------------------------ impulse values
def full_values(rng, n):
    """randn with all 24 mantissa bits in play: values whose mid or lo plane is zero are redrawn (they would not exercise six terms)."""
    out = np.empty(0, F32)
    while out.size < n:
        v = rng.standard_normal(2 * n + 8).astype(F32)
        _, mid, lo = split3(v)
        out = np.concatenate([out, v[(mid != 0) & (lo != 0)]])
    return out[:n]


def exact_values(rng, n):
    """bf16-representable: k / 16 with 1 <= |k| <= 32 and small integers."""
    k = rng.integers(1, 33, n) * rng.choice([-1, 1], n)
    v = np.where(rng.random(n) < 0.7, k / 16.0, rng.integers(1, 4, n)).astype(F32)
    assert is_bf16(v).all()
    return v


def weights(rng, shape, scale=0.2):
    return (rng.standard_normal(shape) * scale).astype(F32)


def out_dim(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def lattice(n, k, phase):
    """Impulse coordinates of pitch k along one axis of length n: anchored at 0 (phase 0) or at n - 1 (phase 1)."""
    return list(range(0, n, k)) if phase == 0 else sorted(range(n - 1, -1, -k))


def _kinds(chan, site, phase, exact_from, group=16):
    """True = full value.  Channel groups of 16 cycle through mixed (alternating by site) / all full / all exact, shifted by the
    lattice phase, so a wave's or block's vote sees all three; a promise route (exact_from >= 0) has full values only below it."""
    if exact_from is not None:
        return (chan < exact_from) & (site % 2 == 0)
    g = (chan // group + phase) % 3
    return (g == 1) | ((g == 0) & (site % 2 == 0))


def impulse_rounds(shape, direction):
    """Launches (rounds) per lattice phase that put an impulse into every contraction channel."""
    B, Cin, Cout, H, W, k, s = shape
    K = Cin if direction == "fwd" else Cout
    SH, SW = (H, W) if direction == "fwd" else (out_dim(H, k, s), out_dim(W, k, s))
    ns = B * min(len(lattice(SH, k, 0)), len(lattice(SH, k, 1))) * min(len(lattice(SW, k, 0)), len(lattice(SW, k, 1)))
    return math.ceil(K / ns)


def impulse_case(shape, direction, phase, rnd, w, exact_from=None, seed=0):
    """One impulse launch of the forward (direction "fwd": src = x [B,H,W,Cin], out = y [B,OH,OW,Cout]) or of the input gradient
    ("dgrad": src = g_y [B,OH,OW,Cout], out = g_x [B,H,W,Cin]).  w: fp32 [Cout,Cin,k,k].  Impulses sit on a lattice of pitch k in
    both image directions of the source (no k x k window holds two, for stride 1 and 2), the impulse of site s in channel
    (s + round) mod K.  -> dict(src, ref (float64, from the fp32 operands), hit (bool: the element is one product), full (bool per
    element: the product's impulse is a full value))."""
    B, Cin, Cout, H, W, k, s = shape
    OH, OW, pad = out_dim(H, k, s), out_dim(W, k, s), k // 2
    fwd = direction == "fwd"
    SH, SW, K = (H, W, Cin) if fwd else (OH, OW, Cout)
    DH, DW, N = (OH, OW, Cout) if fwd else (H, W, Cin)
    ys, xs = lattice(SH, k, phase), lattice(SW, k, phase)
    sites = [(b, y, x) for b in range(B) for y in ys for x in xs]
    ns = len(sites)
    rng = np.random.default_rng([seed, phase, rnd, 1 if fwd else 2])
    idx = np.arange(ns)
    chan = (idx + rnd * ns) % K
    full = _kinds(chan, idx, phase, exact_from)
    val = np.where(full, full_values(rng, ns), exact_values(rng, ns)).astype(F32)
    src = np.zeros((B, SH, SW, K), F32)
    ref = np.zeros((B, DH, DW, N), F64)
    hit = np.zeros((B, DH, DW, N), bool)
    isfull = np.zeros((B, DH, DW, N), bool)
    w64 = np.asarray(w, F64)
    for i, (b, y, x) in enumerate(sites):
        c = int(chan[i])
        src[b, y, x, c] = val[i]
        for ty in range(k):
            for tx in range(k):
                if fwd:  # y[oy, ox] takes x[oy s + ty - pad, ox s + tx - pad] * w[co, c, ty, tx]
                    ny, nx = y + pad - ty, x + pad - tx
                    if ny % s or nx % s:
                        continue
                    dy, dx = ny // s, nx // s
                    col = w64[:, c, ty, tx]
                else:  # g_x[oy s + ty - pad, ox s + tx - pad] takes g_y[oy, ox] * w[c, ci, ty, tx]
                    dy, dx = y * s + ty - pad, x * s + tx - pad
                    col = w64[c, :, ty, tx]
                if 0 <= dy < DH and 0 <= dx < DW:
                    assert not hit[b, dy, dx].any()
                    ref[b, dy, dx] = float(val[i]) * col
                    hit[b, dy, dx] = True
                    isfull[b, dy, dx] = bool(full[i])
    return {"src": src, "ref": ref, "hit": hit, "full": isfull, "nsites": ns, "chan": chan, "val": val}


def wgrad_sites(B, H, W, nsplit, stride=1):
    """Where the weight-gradient impulses sit: the corners, the middle of every edge, an interior pixel, and the first and last
    pixel of each of the nsplit pixel splits (evf_conv2d_wgrad_ws / (9 Cin Cout)) -- in raster order over the batch and in the tile
    order of the two kernels.  The three groups are interleaved, so that a case with few input channels still uses some of each."""
    return _interleave(wgrad_site_groups(B, H, W, nsplit, stride))


def _interleave(groups):
    seen, out = set(), []
    for i in range(max(len(g) for g in groups)):
        for g in groups:
            if i < len(g) and g[i] not in seen:
                seen.add(g[i])
                out.append(g[i])
    return out


def wgrad_site_groups(B, H, W, nsplit, stride=1):
    """-> (corners / edges / interior, split boundaries in raster order, split boundaries in the kernels' tile order)."""
    pts, raster, tiled = [], [], []
    for b in sorted({0, B - 1}):
        pts += [(b, 0, 0), (b, 0, W - 1), (b, H - 1, 0), (b, H - 1, W - 1), (b, 0, W // 2), (b, H - 1, W // 2), (b, H // 2, 0),
                (b, H // 2, W - 1), (b, H // 2, W // 2)]
    npix = B * H * W
    for z in range(max(nsplit, 1)):
        for p in ((z * npix) // max(nsplit, 1), ((z + 1) * npix) // max(nsplit, 1) - 1):
            p = min(max(p, 0), npix - 1)
            raster.append((p // (H * W), (p // W) % H, p % W))
    # ... and of each split in the kernels' own order: a split is a run of pixel tiles (batch, tile row, tile column), 8 x 8 output
    # pixels in k_wgrad9_b3 (WB_T) and (32 / TW) x TW in k_wgrad9 (wg9_plan); the site is the input pixel under the output pixel
    OH, OW = out_dim(H, 3, stride), out_dim(W, 3, stride)
    tw = 32 if OW > 16 else (16 if OW > 8 else 8)
    for th, tc in ((8, 8), (32 // tw, tw)):
        ty, tx = -(-OH // th), -(-OW // tc)
        ntiles = B * ty * tx
        per = -(-ntiles // max(nsplit, 1))
        for z in range(-(-ntiles // per)):
            first, last = z * per, min((z + 1) * per, ntiles) - 1
            for t, corner in ((first, 0), (last, 1)):
                b, r, c = t // (ty * tx), (t // tx) % ty, t % tx
                oy = min(r * th + corner * (th - 1), OH - 1)
                ox = min(c * tc + corner * (tc - 1), OW - 1)
                tiled.append((b, min(oy * stride, H - 1), min(ox * stride, W - 1)))
    return pts, raster, tiled


def wgrad_case(shape, nsplit, kinds="mixed", seed=0):
    """x [B,H,W,Cin] with exactly ONE impulse per input channel over the whole batch, g_y [B,OH,OW,Cout] dense randn: then
    g_w[co,ci,ty,tx] = x_val(ci) * g_y[b, o(t), co] with o(t) the one output pixel whose tap t lands on the site, and exactly 0
    where that pixel is outside the image or of the wrong parity (stride 2).  kinds "mixed": the redo tiles -- 32 * CT input channels, CT = 2
    once Cin > 32 (wg9_plan; the kernels raise one flag per tile) -- alternate between all exact and exactly one full value (the one
    tile of Cin <= 64 holds one: only shapes with Cin > 64 have an all-exact tile BESIDE a flagged one); "exact": all
    bf16-representable.
    -> dict(x, gy, ref [Cout,Cin,k,k] float64, hit, mag = |x g|, bias_ref, bias_abs)."""
    B, Cin, Cout, H, W, k, s = shape
    OH, OW, pad = out_dim(H, k, s), out_dim(W, k, s), k // 2
    rng = np.random.default_rng([seed, 77, Cin, Cout])
    sites = wgrad_sites(B, H, W, nsplit, s)
    ci = np.arange(Cin)
    tw = 64 if Cin > 32 else 32
    tile = ci // tw
    ntile = (Cin + tw - 1) // tw
    full = np.zeros(Cin, bool)
    if kinds == "mixed":
        for t in range(ntile):
            if t % 2 == 1 or ntile == 1:
                width = min(tw, Cin - tw * t)
                full[tw * t + (7 * t + 3) % width] = True
    val = np.where(full, full_values(rng, Cin), exact_values(rng, Cin)).astype(F32)
    x = np.zeros((B, H, W, Cin), F32)
    gy = (rng.standard_normal((B, OH, OW, Cout)) * 0.5).astype(F32)
    ref = np.zeros((Cout, Cin, k, k), F64)
    hit = np.zeros((Cout, Cin, k, k), bool)
    for c in range(Cin):
        b, y, xx = sites[c % len(sites)]
        x[b, y, xx, c] = val[c]
        for ty in range(k):
            for tx in range(k):
                ny, nx = y + pad - ty, xx + pad - tx
                if ny % s or nx % s:
                    continue
                oy, ox = ny // s, nx // s
                if 0 <= oy < OH and 0 <= ox < OW:
                    ref[:, c, ty, tx] = float(val[c]) * gy[b, oy, ox].astype(F64)
                    hit[:, c, ty, tx] = True
    g64 = gy.astype(F64)
    return {"x": x, "gy": gy, "ref": ref, "hit": hit, "full": full, "val": val, "tile": tile, "sites": [sites[c % len(sites)] for c in range(Cin)],
            "bias_ref": g64.sum((0, 1, 2)), "bias_abs": np.abs(g64).sum((0, 1, 2))}


# ------------------------------------------------------------------------------------------------------------ dense references
def conv_fwd64(x, w, s):
    """y [B,OH,OW,Cout] = conv(x [B,H,W,Cin], w [Cout,Cin,k,k]), padding k // 2, stride s, in float64 (direct sum over taps)."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    pad, OH, OW = k // 2, out_dim(H, k, s), out_dim(W, k, s)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, OH, OW, Cout), F64)
    for ty in range(k):
        for tx in range(k):
            y += xp[:, ty:ty + (OH - 1) * s + 1:s, tx:tx + (OW - 1) * s + 1:s] @ w[:, :, ty, tx].T
    return y


def conv_dgrad64(gy, w, s, H, W):
    """g_x [B,H,W,Cin] = conv^T(g_y [B,OH,OW,Cout], w) in float64."""
    gy, w = np.asarray(gy, F64), np.asarray(w, F64)
    B, OH, OW, Cout = gy.shape
    _, Cin, k, _ = w.shape
    pad = k // 2
    gp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    for ty in range(k):
        for tx in range(k):
            gp[:, ty:ty + (OH - 1) * s + 1:s, tx:tx + (OW - 1) * s + 1:s] += gy @ w[:, :, ty, tx]
    return gp[:, pad:pad + H, pad:pad + W]


def conv_wgrad64(x, gy, k, s):
    """g_w [Cout,Cin,k,k] = sum over pixels of g_y (x) x shifted, in float64."""
    x, gy = np.asarray(x, F64), np.asarray(gy, F64)
    B, H, W, Cin = x.shape
    _, OH, OW, Cout = gy.shape
    pad = k // 2
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    gw = np.zeros((Cout, Cin, k, k), F64)
    g2 = gy.reshape(-1, Cout)
    for ty in range(k):
        for tx in range(k):
            gw[:, :, ty, tx] = g2.T @ xp[:, ty:ty + (OH - 1) * s + 1:s, tx:tx + (OW - 1) * s + 1:s].reshape(-1, Cin)
    return gw


def dense_inputs(rng, shape, kind):
    """x of the dense leg: "real" randn, "spikes" (small sums and blends of spikes: multiples of 1/16), "mixed" (spikes behind a
    real-valued head of four channels)."""
    if kind == "real":
        return rng.standard_normal(shape).astype(F32)
    x = (rng.integers(0, 33, shape) / 16.0 * (rng.random(shape) < 0.4)).astype(F32)
    if kind == "mixed":
        h = min(4, shape[-1])
        x[..., :h] = rng.standard_normal(shape[:-1] + (h,)).astype(F32)
    return x


def emulate_dense_fwd(x, w, s, nslab=1, mutate=None):
    """fp32 forward in the kernels' association: stages (tap, 16-channel chunk) in index order, per stage the six split terms in issue
    order, each term one matrix instruction = the exact sum of its 16 products added to the fp32 accumulator with one rounding; the
    stages cut into nslab slabs that are then added in index order.  mutate: "border" reads the nearest pixel instead of the zero
    padding (a wrong tap at the image border), "tail" leaves out the last input channel (a ragged group's last channel)."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    pad, OH, OW = k // 2, out_dim(H, k, s), out_dim(W, k, s)
    if mutate == "tail":
        x = x.copy()
        x[..., Cin - 1] = 0
    xs = []
    for plane in split3(x):
        xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
        xp[:, pad:pad + H, pad:pad + W] = plane
        if mutate == "border" and pad:
            xp = np.pad(plane.astype(F64), ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="edge")
        xs.append(xp)
    ws = [p.astype(F64) for p in split3(w)]
    stages = [(ty, tx, c0) for ty in range(k) for tx in range(k) for c0 in range(0, Cin, 16)]
    per = math.ceil(len(stages) / nslab)
    slabs = []
    for z in range(nslab):
        acc = np.zeros((B, OH, OW, Cout), F32)
        for ty, tx, c0 in stages[z * per:(z + 1) * per]:
            for i, j in TERMS6:
                part = xs[i][:, ty:ty + (OH - 1) * s + 1:s, tx:tx + (OW - 1) * s + 1:s, c0:c0 + 16] @ ws[j][:, c0:c0 + 16, ty, tx].T
                acc = (acc.astype(F64) + part).astype(F32)
        slabs.append(acc)
    y = slabs[0]
    for z in range(1, nslab):
        y = (y + slabs[z]).astype(F32)
    return y


def dense_units(got, ref, scale):
    """|got - ref| in units of 2^-24 * scale, elementwise (0 where both vanish)."""
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    scale = np.asarray(scale, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / (U * scale), np.where(err > 0, np.inf, 0.0))
