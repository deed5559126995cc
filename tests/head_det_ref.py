"""References of the three fixed-order sums a voxel-input FireNet step reaches in deterministic mode: evf_head_wgrad_det (the head
convolution's weight gradient for a real-valued input of any channel count), evf_lif_bwd_det (the per-channel leak / threshold
sums of the stand-alone neuron backward) and evf_norm_nonzero_det (norm_input's statistics).  For each: the case list, seeded
inputs shared by the CPU and the GPU tests, the float64 reference with the scale of its bound, a Python mirror of the launch
geometry and the CHAIN LENGTH counted from it (the largest number of additions a term passes through -- not measured).  Not a
test module itself.

Bounds, in units of U * sum |terms| (U = 2^-24): every addition of a chain rounds once and errs by at most U times the partial sum
it forms, itself at most sum |terms| (1 + small), so `chain` additions cost `chain` units to first order; a term formed by `ops`
rounded operations carries `ops` more (each operation's relative error counted against the MAGNITUDES it combines, so that a
cancelling difference is covered).  Bound = ops + chain.  Nothing here is fitted to what a kernel returns.  conv_ref.K_SUM is not
imported: it is twice the emulated error of other kernels' association, not a count that carries over to these."""

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
C = 32


def cdiv(a, b):
    return -(-a // b)


def sum_rows_chain(nrows):
    """evf_sum_rows(accumulate = 0), k_sum_rows: group g adds rows g, g + 16, ... in order, then the 16 groups in order."""
    return cdiv(nrows, 16) + 16


def units(got, ref, scale):
    """Largest |got - ref| / (U * scale) over the elements with a non-zero scale; inf when an element of scale zero differs or the
    non-finite patterns differ."""
    got, ref, scale = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(scale, F64)
    if not np.array_equal(np.isfinite(got), np.isfinite(ref)):
        return np.inf
    fin = np.isfinite(ref)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    zero = scale == 0
    if (err[zero] != 0).any():
        return np.inf
    if zero.all():
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())


# ================================================================================================================ head wgrad
# (B, Cin, H, W): one block with an idle wave and W < 8; ...; 36 rows = two M tiles and a W tail; 45 rows; 72 rows = three
# tiles with the rr < nrow edge; Cin = 2; B * H / 4 = 260 > 256: the grid cap and a second grid-stride trip
HEAD_CASES = ((1, 1, 3, 5), (2, 3, 5, 8), (1, 4, 6, 13), (2, 5, 7, 20), (1, 8, 4, 9), (3, 2, 9, 16), (5, 5, 208, 8))
HEAD_BLOCK_CAP = 256


def head_wgrad_det_slabs(B, H, W):
    """Grid of k_head_wgrad (both forms) = rows of the slab: four image rows per block and trip, at most 256 blocks."""
    return min(cdiv(B * H, 4), HEAD_BLOCK_CAP)


def head_chain(B, Cin, H, W, calls=1):
    """A wave walks ceil(B * H / (4 * blocks)) image rows; a row is ceil(W / 8) steps of four MFMAs with K = 2 (two additions
    each, padding zeros included); then (w0 + w1) + (w2 + w3); a second call adds onto the slab row; then evf_sum_rows."""
    nb = head_wgrad_det_slabs(B, H, W)
    rows_per_wave = cdiv(B * H, 4 * nb)
    return rows_per_wave * cdiv(W, 8) * 8 * calls + 2 * calls + (calls - 1) + sum_rows_chain(nb)


HEAD_OPS = 1  # the product


def head_bound(B, Cin, H, W, calls=1):
    return HEAD_OPS + head_chain(B, Cin, H, W, calls)


def _seed(*key):
    return np.random.default_rng([int(k) for k in key])


def head_inputs(case, leg, rep=0):
    """x [B,Cin,H,W], g_cur [B,H,W,32] (float32).  leg "exact": integers in [-3, 3] and multiples of 2^-6 in [-2, 2] -- every
    product and every partial sum of at most 2^15 of them is exactly representable; "real": normal data."""
    B, Cin, H, W = case
    rng = _seed(B, Cin, H, W, 1 if leg == "exact" else 2, rep)
    if leg == "exact":
        x = rng.integers(-3, 4, (B, Cin, H, W)).astype(F32)
        g = (rng.integers(-128, 129, (B, H, W, C)) / 64.0).astype(F32)
    else:
        x = rng.standard_normal((B, Cin, H, W)).astype(F32)
        x[rng.random(x.shape) < 0.3] = 0.0  # (a voxel grid has empty pixels)
        g = (0.1 * rng.standard_normal((B, H, W, C))).astype(F32)
    return x, g


def head_wgrad_ref64(x, g, drop_tap=None, drop_channel=None):
    """dW [32][Cin][3][3] = sum_pix g[pix][co] * x[b][ci][pix + tap] (zero padding) in float64, and sum |g| |x| per element.
    drop_tap = (b, y, x_, ci, ky, kx): that one term is left out (of every co); drop_channel = co: that output channel's
    terms of the last pixel are left out -- the mutants the CPU test holds the bound against."""
    x, g = np.asarray(x, F64), np.asarray(g, F64)
    B, Cin, H, W = x.shape
    xp = np.zeros((B, Cin, H + 2, W + 2), F64)
    xp[:, :, 1:-1, 1:-1] = x
    dw, sc = np.zeros((C, Cin, 3, 3), F64), np.zeros((C, Cin, 3, 3), F64)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + H, kx:kx + W]
            dw[:, :, ky, kx] = np.einsum("bhwo,bchw->oc", g, xs)
            sc[:, :, ky, kx] = np.einsum("bhwo,bchw->oc", np.abs(g), np.abs(xs))
    if drop_tap is not None:
        b, y, x_, ci, ky, kx = drop_tap
        dw[:, ci, ky, kx] -= g[b, y, x_, :] * xp[b, ci, y + ky, x_ + kx]
    if drop_channel is not None:
        co = drop_channel
        dw[co] -= g[B - 1, H - 1, W - 1, co] * xp[B - 1, :, H - 1:H + 2, W - 1:W + 2]
    return dw, sc


# ================================================================================================================ lif backward
# (B, H, W, nrows): less than one block of work; a few blocks; the default rule gives 768 blocks, the cap to 512 rows forces a
# second grid-stride trip; three rows for 80 blocks' worth of work
LIF_CASES = ((1, 3, 5, 512), (2, 32, 40, 512), (1, 160, 160, 512), (2, 32, 40, 3))
LIF_BLOCK_CAP = 768
ARCTAN, SUPERSPIKE = 0, 1
WIDTH = {ARCTAN: 10.0, SUPERSPIKE: 10.0}
LEAK_MAX = 1.5  # |leak| of the generated cases: lam / (1 - lam) <= e^1.5
THRESH_FLOOR_CHANNEL = 7  # the channel whose thresh sits AT the 0.01 floor: clamp_min passes no gradient there


def lif_bwd_grid(B, H, W, nrows=None):
    """evf_lif_bwd: one float4 (four channels of a pixel) per thread and trip, at most 768 blocks; the twin: ... and nrows."""
    g = min(cdiv(B * H * W * 8, 256), LIF_BLOCK_CAP)
    return g if nrows is None else min(g, nrows)


def lif_chain(B, H, W, nrows):
    """trips of a thread + three shuffle levels (lanes 8, 16, 32 apart) + four waves + the add onto the row + evf_sum_rows over
    all nrows rows (the rows behind the grid hold zeros and are still added)."""
    nb = lif_bwd_grid(B, H, W, nrows)
    return cdiv(B * H * W * 8, nb * 256) + 3 + 4 + 1 + sum_rows_chain(nrows)


def lif_ops(kappa):
    """Rounded operations behind one term, each relative to the magnitudes of lif_bwd_ref64's scale:
      sg   : v - th, x * x, * w, 1 + ., v_rcp_f32 (1 ulp = 2 U)                                            <= 8   (positive sum)
      gv   : g_z * sg, g_v + .                                                                             <= 10
      lam  : expf (1 ulp = 2 U, allowed 4), 1 + ., 1 / .                                                    <= 6
      oml  : 1 - lam carries lam's error lam / oml = kappa times over, plus its own rounding              <= 6 kappa + 1
      cur  : v_prev * lam (lam's 6 + 1), v - ., (+ z * th, soft: 2), 1 / oml (2), * .                      <= 13 + (6 kappa + 1)
      leak : dlam's subtraction, gv * dlam (gv's 10 + 1), * l (6 + 1), * (1 - l) (6 kappa + 1 + 1)          <= 21 + 6 kappa + cur
      thresh: g_z * sg (9) or gv * z (11), the subtraction from the running sum is the chain's              <= 11"""
    leak = 21 + 6 * kappa + 13 + 6 * kappa + 1
    return {"leak": leak, "thresh": 11}


def lif_bound(case, which):
    B, H, W, nrows = case
    return lif_ops(np.exp(LEAK_MAX))[which] + lif_chain(B, H, W, nrows)


def lif_inputs(case, first=False, rep=0):
    """Tape and upstream gradients of one pass, float32: g_z, g_v, v_out, v_prev [npix,32], z_prev (bits, uint32 [npix]), leak,
    thresh [32].  first: the window's first pass in backward order has no g_v; v_prev / z_prev absent = zero state."""
    B, H, W, _ = case
    npix = B * H * W
    rng = _seed(B, H, W, 3, rep)
    thresh = (0.2 + 0.6 * rng.random(C)).astype(F32)
    thresh[THRESH_FLOOR_CHANNEL] = 0.01
    leak = rng.uniform(-LEAK_MAX, LEAK_MAX, C).astype(F32)
    d = {"g_z": (0.5 * rng.standard_normal((npix, C))).astype(F32), "g_v": (0.5 * rng.standard_normal((npix, C))).astype(F32),
         "v_out": (0.5 * rng.standard_normal((npix, C)) + 0.3).astype(F32), "v_prev": (0.5 * rng.standard_normal((npix, C))).astype(F32),
         "z_prev": rng.integers(0, 2 ** 32, npix, dtype=np.uint64).astype(np.uint32), "leak": leak, "thresh": thresh}
    if first:
        d["g_v"] = d["v_prev"] = d["z_prev"] = None
    return d


def lif_exact_inputs(case, rep=0):
    """The exact leg of the row sums: leak = 0 in every channel (lam = 1 / (1 + exp(0)) = 0.5, 1 / (1 - lam) = 2 and the factor
    l (1 - l) = 0.25, all exact), thresholds in {0.25, 0.5}, v_out AT the threshold (the surrogate's argument is 0: sg = 1 / 1),
    v_prev multiples of 1/4 in [-1, 1], g_z / g_v multiples of 1/8 in [-1, 1].  Every term of g_leak is then a multiple of 2^-5
    of magnitude <= 6 and every term of g_thresh a multiple of 1/8 of magnitude <= 3: all partial sums of up to 2^16 pixels are
    exact in float32, in any order.  The floor channel (thresh = 0.01, not dyadic) gets v_out = 0.25, g_z = 0 and no previous
    spike, so its spike gradient is 0 * sg = 0 exactly, the soft reset's z * th vanishes and its terms stay dyadic."""
    B, H, W, _ = case
    npix = B * H * W
    rng = _seed(B, H, W, 4, rep)
    thresh = rng.choice(np.array([0.25, 0.5], F32), C).astype(F32)
    thresh[THRESH_FLOOR_CHANNEL] = 0.01
    v_out = np.broadcast_to(np.where(thresh > 0.1, thresh, F32(0.25)), (npix, C)).astype(F32)
    g_z = (rng.integers(-8, 9, (npix, C)) / 8.0).astype(F32)
    g_z[:, THRESH_FLOOR_CHANNEL] = 0.0
    return {"g_z": g_z, "g_v": (rng.integers(-8, 9, (npix, C)) / 8.0).astype(F32), "v_out": v_out,
            "v_prev": (rng.integers(-4, 5, (npix, C)) / 4.0).astype(F32),
            "z_prev": rng.integers(0, 2 ** 32, npix, dtype=np.uint64).astype(np.uint32) & np.uint32(~(1 << THRESH_FLOOR_CHANNEL) & 0xFFFFFFFF),
            "leak": np.zeros(C, F32), "thresh": thresh}


def surrogate64(kind, x, width):
    if kind == ARCTAN:
        return 1.0 / (1.0 + width * x * x)  # spiking_util.py:88-93
    return 1.0 / (1.0 + width * np.abs(x)) ** 2  # :38-43


def unpack_bits(z, npix):
    if z is None:
        return np.zeros((npix, C), F64)
    return ((np.asarray(z, np.uint32)[:, None] >> np.arange(C, dtype=np.uint32)[None, :]) & 1).astype(F64)


def lif_bwd_ref64(d, hard, surrogate, nblk, v_out64=None):
    """float64 statement of k_lif_bwd on the float32 inputs `d` (None entries = absent): g_cur, g_v_prev [npix,32]; the per-BLOCK
    rows [nblk,32] of g_leak / g_thresh with l (1 - l) and the thresh > 0.01 gate applied PER BLOCK, where the kernel applies them
    (element e = 8 pix + c / 4 belongs to block (e / 256) mod nblk); their sums over the blocks; and per channel the scales
    sum of magnitudes (see lif_ops).  v_out64: a float64 potential in place of d["v_out"] (the CPU test against autograd)."""
    vo = np.asarray(d["v_out"], F64) if v_out64 is None else v_out64
    npix = vo.shape[0]
    z64 = lambda a: np.zeros((npix, C), F64) if a is None else np.asarray(a, F64)  # noqa: E731
    gz, gvo, vp = z64(d["g_z"]), z64(d["g_v"]), z64(d["v_prev"])
    z = unpack_bits(d["z_prev"], npix)
    lam = 1.0 / (1.0 + np.exp(-np.asarray(d["leak"], F64)))
    th = np.maximum(np.asarray(d["thresh"], F64), 0.01)
    oml = 1.0 - lam
    sg = surrogate64(surrogate, vo - th, WIDTH[surrogate])
    gsp = gz * sg
    gv = gvo + gsp
    G = np.abs(gvo) + np.abs(gsp)
    if hard:
        gp = gv * lam * (1.0 - z)
        cur = (vo - vp * lam * (1.0 - z)) / oml
        dlam = vp * (1.0 - z) - cur
        mag = np.abs(vp) * (1.0 - z) + (np.abs(vo) + np.abs(vp) * lam * (1.0 - z)) / oml
        t_th, m_th = -gsp, np.abs(gsp)
    else:
        gp = gv * lam
        cur = (vo - vp * lam + z * th) / oml
        dlam = vp - cur
        mag = np.abs(vp) + (np.abs(vo) + np.abs(vp) * lam + z * th) / oml
        t_th, m_th = -gsp - gv * z, np.abs(gsp) + G * z
    t_lk, m_lk = gv * dlam, G * mag
    blk = ((np.arange(npix * 8) // 256) % nblk).repeat(4).reshape(npix, C)  # block of every (pixel, channel)
    slot = (blk * C + np.arange(C)[None, :]).reshape(-1)
    rows_l = np.bincount(slot, weights=t_lk.reshape(-1), minlength=nblk * C).reshape(nblk, C)
    rows_t = np.bincount(slot, weights=t_th.reshape(-1), minlength=nblk * C).reshape(nblk, C)
    rows_l *= lam * (1.0 - lam)                              # d sigmoid, per block
    rows_t *= (np.asarray(d["thresh"], F32) > F32(0.01))     # clamp_min's gate, per block
    return {"g_cur": gv * oml, "g_v_prev": gp, "rows_leak": rows_l, "rows_thresh": rows_t,
            "g_leak": rows_l.sum(0), "g_thresh": rows_t.sum(0),
            "scale_leak": m_lk.sum(0) * lam * (1.0 - lam), "scale_thresh": m_th.sum(0)}


# ================================================================================================================ norm_input
NORM_N = (1, 2, 255, 1024, 1025, 2 ** 20 + 5)  # the last: 1025 blocks' worth of data on 1024 blocks
NORM_BLOCK_CAP = 1024
# out = (v - mean) / sd in float32 from the float64 statistics: mean rounded to float32 (1, against |mean|), the subtraction (1),
# sd rounded (1), the division (correctly rounded or 1 ulp: 2), all against (|v| + |mean|) / sd; the float64 sums behind mean and
# sd pass through fewer than 2^11 additions of 2^-53 each, far below one U: 1 more
NORM_OPS = 6


def norm_grid(n):
    """1024 elements per block and trip (256 threads, four trips), at most 1024 blocks."""
    return min(cdiv(n, 1024), NORM_BLOCK_CAP)


def norm_ws(n):
    return 3 * norm_grid(n)


def norm_inputs(n, kind):
    """"voxel": ~70 % zeros, some of them -0.0; "zeros"; "one": exactly one non-zero entry."""
    rng = _seed(n, 5)
    if kind == "zeros":
        return np.zeros(n, F32)
    if kind == "one":
        x = np.zeros(n, F32)
        x[n // 2] = 1.75
        x[::3] *= F32(-1.0)  # (-0.0 among the zeros, or a negative entry: either way one non-zero)
        return x
    x = (0.8 * rng.standard_normal(n) + 0.2).astype(F32)
    x[rng.random(n) < 0.7] = 0.0
    x[rng.random(n) < 0.1] *= F32(-1.0)  # -0.0 where it was zero
    return x


def norm_ref64(x):
    """models/model.py:247-252 in float64 -> (out, scale): zero entries stay +0.0; fewer than two non-zero entries: NaN there."""
    x = np.asarray(x, F64)
    nz = x != 0
    out, scale = np.zeros(x.shape, F64), np.zeros(x.shape, F64)
    k = int(nz.sum())
    if k == 0:
        return out, scale
    if k == 1:
        out[nz] = np.nan
        return out, scale
    m = x[nz].mean()
    sd = np.sqrt(((x[nz] - m) ** 2).sum() / (k - 1))
    out[nz] = (x[nz] - m) / sd
    scale[nz] = (np.abs(x[nz]) + abs(m)) / sd
    return out, scale
