"""References of the deterministic sums of the non-spiking zoo: evf_chan_reduce_det (per-channel statistics of batch / instance /
group norm, and the bias gradient of every convolution), evf_leaky_bwd_det (g_leak of the leaky cells) and evf_conv2d_wgrad_det
(the generic-kernel-size weight gradient).  For every entry point: the shared, seeded inputs of the CPU and the GPU tests, the
float64 reference with the scale of its bound, the geometry twin (blocks, rows, runs and the CHAIN LENGTH: the largest number
of additions a term passes through, counted from the launch rule of the host wrapper, not measured) and a float32 emulation of
the kernels' association in numpy.  Not a test module itself.

Bounds, in units of 2^-24 * sum |terms|: every addition of a chain rounds once and errs by at most 2^-24 of the partial sum it
forms, itself at most sum |terms| (1 + small): chain additions cost `chain` units to first order.  A term formed by `ops` rounded
operations carries `ops` more.  chan_reduce: ops + chain (ops = 0 / 2 / 3 for the three modes).  g_leak: the bound of the default
entry's test, K_LEAKY + chain, with this twin's chain.  Bias and weight gradient: the project's own bar K_SUM of
tests/conv_ref.py, whatever the chain."""

import numpy as np

import conv_ref as CR
import neuron_gen_ref as R

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
RUNS = 16  # runs of consecutive rows per column in every row-sum launch (CR_RUNS, NG_RS_GROUPS, WGR_G)
CHAN_OPS = {0: 0, 1: 2, 2: 3}


def cdiv(a, b):
    return -(-a // b)


def rowsum32(rows, init=None):
    """The row-sum launches: rows [nrows, ...] float32 -> 16 runs of consecutive rows, each added in row order from 0, the runs
    in run order from 0; `init`: the sum is added onto it."""
    rows = np.asarray(rows, F32)
    n = rows.shape[0]
    per = cdiv(n, RUNS)
    runs = []
    for r in range(RUNS):
        t = np.zeros(rows.shape[1:], F32)
        for i in range(r * per, min(r * per + per, n)):
            t = (t + rows[i]).astype(F32)
        runs.append(t)
    a = np.zeros(rows.shape[1:], F32)
    for t in runs:
        a = (a + t).astype(F32)
    return a if init is None else (np.asarray(init, F32) + a).astype(F32)


# ================================================================================================================ chan_reduce
CHAN_C = (3, 32, 96)  # not a power of two, one channel pass, the c0 loop
CHAN_NPG = (5, 700, 40000)  # fewer pixels than pixel lanes, a few blocks, many blocks per group
CHAN_G = (1, 3)


def chan_geometry(G, npg, C):
    """Launch rule of evf_chan_reduce: 256 threads = npl pixel lanes x ct channel lanes (ct = min(C, 64) rounded up to a power of
    two); at most 2048 / G blocks per group, at least 8 pixels per pixel lane; a block walks ppb pixels of one group."""
    ct = 1
    while ct < C and ct < 64:
        ct <<= 1
    npl = 256 // ct
    bpg = max(min(cdiv(2048, G), cdiv(npg, npl * 8)), 1)
    ppb = cdiv(npg, bpg)
    bpg = cdiv(npg, ppb)
    per = cdiv(bpg, RUNS)
    chain = cdiv(ppb, npl) + npl + per + RUNS + 1  # thread's loop, the pixel lanes, a run, the runs, onto the output
    return {"ct": ct, "npl": npl, "bpg": bpg, "ppb": ppb, "blocks": bpg * G, "rows": bpg, "cols": C, "runs": RUNS, "per": per,
            "chain": chain}


def chan_inputs(G, npg, C, pad):
    """x [G * npg, C + pad], y likewise, center / scale [G, C], out_init [G, C] (all float32; the padding columns hold 1e6)."""
    rng = np.random.default_rng(1000 * G + 7 * npg + C + pad)
    ld = C + pad
    x = np.full((G * npg, ld), 1e6, F32)
    y = np.full((G * npg, ld), 1e6, F32)
    x[:, :C] = rng.normal(0.3, 1.0, (G * npg, C))
    y[:, :C] = rng.normal(0.0, 1.0, (G * npg, C))
    center = rng.normal(0.3, 0.1, (G, C)).astype(F32)
    scale = rng.uniform(0.5, 2.0, (G, C)).astype(F32)
    init = rng.normal(0, 3, (G, C)).astype(F32)
    return x, y, center, scale, init


def _chan_terms(x, y, center, scale, mode, G, npg, C, dtype):
    v = np.asarray(x[:, :C], dtype).reshape(G, npg, C)
    if mode == 0:
        return v
    d = (v - np.asarray(center, dtype)[:, None, :]).astype(dtype)
    if mode == 1:
        return (d * d).astype(dtype)
    w = np.asarray(y[:, :C], dtype).reshape(G, npg, C)
    return (w * (d * np.asarray(scale, dtype)[:, None, :]).astype(dtype)).astype(dtype)


def chan_ref64(x, y, center, scale, mode, G, npg, C):
    """-> (sums [G, C], sum |terms| [G, C]) in float64."""
    t = _chan_terms(x, y, center, scale, mode, G, npg, C, F64)
    return t.sum(1), np.abs(t).sum(1)


def chan_emulate32(x, y, center, scale, mode, G, npg, C, init=None):
    """k_chan_reduce<DET> + k_chan_rowsum in float32: a thread's strided loop, the pixel lanes in lane order, the rows."""
    g = chan_geometry(G, npg, C)
    npl, ppb, bpg = g["npl"], g["ppb"], g["bpg"]
    t = _chan_terms(x, y, center, scale, mode, G, npg, C, F32)
    trips = cdiv(ppb, npl)
    pad = np.zeros((G, bpg * ppb, C), F32)
    pad[:, :npg] = t
    blk = np.zeros((G, bpg, trips * npl, C), F32)
    blk[:, :, :ppb] = pad.reshape(G, bpg, ppb, C)
    blk = blk.reshape(G, bpg, trips, npl, C)
    acc = np.zeros((G, bpg, npl, C), F32)
    for j in range(trips):
        acc = (acc + blk[:, :, j]).astype(F32)
    rows = np.zeros((G, bpg, C), F32)
    for q in range(npl):
        rows = (rows + acc[:, :, q]).astype(F32)
    out = np.stack([rowsum32(rows[i]) for i in range(G)])
    return out if init is None else (np.asarray(init, F32) + out).astype(F32)


# ================================================================================================================= bias use
BIAS_COUT = (2, 24, 130)
BIAS_M = 2 * 20 * 24


def bias_inputs(Cout):
    """g_y [M, ldg] with ldg > Cout (padding 1e6) and the initial contents of g_bias."""
    rng = np.random.default_rng(Cout)
    ldg = (Cout + 7) // 4 * 4
    gy = np.full((BIAS_M, ldg), 1e6, F32)
    gy[:, :Cout] = rng.standard_normal((BIAS_M, Cout)) * 0.5
    return gy, rng.normal(0, 3, Cout).astype(F32)


# =================================================================================================================== leaky
LEAKY_ACTS = ((0, None), (3, "relu"), (1, "tanh"))  # (evf_act id, name)
LEAKY_UPSTREAM = ("both", "out", "state")


def leaky_geometry(C, npix):
    """Launch rule of evf_leaky_bwd: the block of evf_neuron_bwd ((256 / Q) * Q threads, 256 from Q = 256 on), one float4 per
    thread and trip, at most 1024 blocks.  In the block (DET): Q >= 64 the block / Q owners of a channel quad add in turns; Q a
    smaller power of two: log2(64 / Q) shuffle levels, then one slot per wave; otherwise one slot per group of Q threads."""
    b = R.bwd_geometry(C, npix)
    Q, bs, np2 = b["Q"], b["bs"], b["np2"]
    total = npix * Q
    nblk = min(cdiv(total, bs), 1024)
    trips = cdiv(total, nblk * bs)
    if Q >= 64:
        arm, inblock = "turns", bs // Q
    elif np2:
        arm, inblock = "groups", bs // Q
    else:
        arm, inblock = "shuffle", int(np.log2(64 // Q)) + cdiv(bs, 64)
    per = cdiv(nblk, RUNS)
    return {"Q": Q, "bs": bs, "nblk": nblk, "trips": trips, "np2": np2, "arm": arm, "rows": nblk, "cols": C, "runs": RUNS,
            "per": per, "chain": trips + inblock + per + RUNS + 1}


def leaky_inputs(C, npix):
    rng = np.random.default_rng(C * 31 + npix)
    n = (npix, C)
    u = lambda: rng.uniform(-2, 2, n).astype(F32)  # noqa: E731
    return {"cur": u(), "prev": u(), "g_out": rng.normal(0, 1, n).astype(F32), "g_state": rng.normal(0, 1, n).astype(F32),
            "leak": rng.uniform(-4, 4, C).astype(F32), "init": rng.normal(0, 3, C).astype(F32)}


def leaky_mix32(cur, prev, leak):
    """evf_leaky_fwd's mix in float32 numpy (the CPU stand-in for the device's own mix)."""
    lam = R._sig32(np.asarray(leak, F32))
    p = np.zeros_like(cur) if prev is None else prev
    return ((p * lam).astype(F32) + ((F32(1) - lam).astype(F32) * cur).astype(F32)).astype(F32)


def leaky_reference(mix32, prev, leak, act, g_out, g_state):
    """The float64 gradients of the update that yields exactly `mix32` (as tests/test_gpu_neuron_gen.py does)."""
    m = np.asarray(mix32, F64)
    lam = 1 / (1 + np.exp(-np.asarray(leak, F64)))
    cur_rec = (m - (np.asarray(prev, F64) if prev is not None else 0.0) * lam) / (1 - lam)
    return R.leaky_ref(cur_rec, prev, None, leak, act, g_out=g_out, g_state=g_state)


def _act32(act, v):
    if act == "tanh":
        return np.tanh(v).astype(F32)
    if act == "sigmoid":
        return (F32(1) / (F32(1) + np.exp(-v).astype(F32))).astype(F32)
    if act == "relu":
        return np.maximum(v, F32(0))
    return v


def _dact32(act, o):
    if act == "tanh":
        return (F32(1) - (o * o).astype(F32)).astype(F32)
    if act == "sigmoid":
        return (o * (F32(1) - o).astype(F32)).astype(F32)
    if act == "relu":
        return (o > 0).astype(F32)
    return np.ones_like(o)


def leaky_emulate32(mix32, prev, leak, act, g_out, g_state, init):
    """g_leak of k_leaky_bwd<DET> + k_neuron_rowsum in float32: a thread's trips, the block's arm, the rows, onto `init`."""
    npix, C = mix32.shape
    g = leaky_geometry(C, npix)
    Q, bs, nblk, trips = g["Q"], g["bs"], g["nblk"], g["trips"]
    lam = R._sig32(np.asarray(leak, F32))
    oml = (F32(1) - lam).astype(F32)
    m = np.asarray(mix32, F32)
    p = np.zeros_like(m) if prev is None else np.asarray(prev, F32)
    go = np.zeros_like(m) if g_out is None else np.asarray(g_out, F32)
    gs = np.zeros_like(m) if g_state is None else np.asarray(g_state, F32)
    G = (gs + (go * _dact32(act, _act32(act, m))).astype(F32)).astype(F32)
    c = ((m - (p * lam).astype(F32)).astype(F32) / oml).astype(F32)
    term = (G * (p - c).astype(F32)).astype(F32).reshape(npix * Q, 4)
    pad = np.zeros((trips * nblk * bs, 4), F32)
    pad[:npix * Q] = term
    pad = pad.reshape(trips, nblk, bs, 4)
    s0 = np.zeros((nblk, bs, 4), F32)
    for j in range(trips):
        s0 = (s0 + pad[j]).astype(F32)
    f = lambda s: ((s * lam.reshape(Q, 4)).astype(F32) * oml.reshape(Q, 4)).astype(F32)  # noqa: E731  (s [.., Q, 4])
    if g["arm"] == "shuffle":
        w = s0.reshape(nblk, bs // 64, 64, 4)
        lane = np.arange(64)
        o = Q
        while o < 64:
            w = (w + w[:, :, lane ^ o]).astype(F32)
            o <<= 1
        slots = f(w[:, :, :Q])  # [nblk, waves, Q, 4]
    else:
        slots = f(s0.reshape(nblk, bs // Q, Q, 4))
    rows = np.zeros((nblk, Q, 4), F32)
    for t in range(slots.shape[1]):
        rows = (rows + slots[:, t]).astype(F32)
    return rowsum32(rows.reshape(nblk, C), init)


# =================================================================================================================== wgrad
# (B, H, W, Cin, Cout, k, stride): K splits > 1, both CT / NT = 2 tiles, unaligned channel counts
WGRAD_SHAPES = ((2, 20, 24, 9, 11, 5, 1), (2, 20, 24, 40, 36, 5, 2), (1, 24, 24, 12, 12, 7, 1), (2, 20, 24, 48, 8, 1, 1))
WGRAD_OFFSET_CASE = ((2, 20, 24, 12, 36, 5, 1), 20, 5)  # (shape, cin_total, cin_off): accumulate = 1 onto a random g_w
WGRAD_FORWARD_CASE = (2, 20, 24, 12, 16, 3, 1)


def wgrad_det_geometry(B, H, W, Cin, Cout, k, s):
    """Split rule of evf_conv2d_wgrad's generic-kernel-size path: (32 CT) x (32 NT) weight tiles per tap, about 1024 blocks, at
    least 8 stages of 32 pixels per split.  A wave multiplies 8 of a stage's 32 pixels (4 matrix instructions of 2 pixels)."""
    M = B * CR.out_dim(H, k, s) * CR.out_dim(W, k, s)
    CT, NT = (2 if Cin > 32 else 1), (2 if Cout > 32 else 1)
    T = k * k
    tiles = cdiv(Cin, 32 * CT) * cdiv(Cout, 32 * NT) * T
    st_total = cdiv(M, 32)
    ksplit = max(min(cdiv(1024, tiles), st_total // 8), 1)
    stages = cdiv(st_total, ksplit)
    ksplit = cdiv(st_total, stages)
    per = cdiv(ksplit, RUNS)
    chain = stages * 8 + 4 + per + RUNS + 1  # a wave's products, the four waves, a run, the runs, onto the output
    return {"M": M, "CT": CT, "NT": NT, "T": T, "ksplit": ksplit, "stages": stages, "blocks": ksplit * (tiles // T) * T,
            "rows": ksplit, "cols": T * Cin * Cout, "runs": RUNS, "per": per, "chain": chain}


def wgrad_inputs(shape, ldx_pad=0):
    B, H, W, Cin, Cout, k, s = shape
    rng = np.random.default_rng(Cin + 3 * Cout + k)
    OH, OW = CR.out_dim(H, k, s), CR.out_dim(W, k, s)
    x = rng.standard_normal((B, H, W, Cin + ldx_pad)).astype(F32)
    gy = (rng.standard_normal((B, OH, OW, Cout)) * 0.5).astype(F32)
    return x, gy


def _im2col(x, k, s):
    """[M, T, Cin] float64: the input value under tap t of output pixel m (0 outside the image)."""
    B, H, W, Cin = x.shape
    OH, OW, pad = CR.out_dim(H, k, s), CR.out_dim(W, k, s), k // 2
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = np.empty((B, OH, OW, k * k, Cin), F64)
    for dy in range(k):
        for dx in range(k):
            cols[:, :, :, dy * k + dx] = xp[:, dy:dy + (OH - 1) * s + 1:s, dx:dx + (OW - 1) * s + 1:s]
    return cols.reshape(B * OH * OW, k * k, Cin)


def wgrad_emulate32(x, gy, k, s, init=None):
    """k_conv2d_wgrad_f32<SLAB> + k_wgrad_reduce_taps in float32: a matrix instruction = the exact sum of its two products added
    to the accumulator with one rounding (the convention of conv_ref.emulate_dense_fwd); wave w of a block takes pixel pairs w,
    w + 4, w + 8, w + 12 of every 32-pixel stage; the four waves in wave order; the splits by rowsum32.  -> [Cout, Cin, k, k]."""
    B, H, W, Cin = x.shape
    Cout = gy.shape[-1]
    g = wgrad_det_geometry(B, H, W, Cin, Cout, k, s)
    M, T, ksplit, stages = g["M"], g["T"], g["ksplit"], g["stages"]
    cols = np.zeros((ksplit * stages * 32, T * Cin), F64)
    cols[:M] = _im2col(x, k, s).reshape(M, T * Cin)
    gf = np.zeros((ksplit * stages * 32, Cout), F64)
    gf[:M] = np.asarray(gy, F64).reshape(M, Cout)
    pr = cols[:, :, None] * gf[:, None, :]  # exact products of float32 values in float64
    pairs = (pr[0::2] + pr[1::2]).reshape(ksplit, stages, 4, 4, T * Cin, Cout)  # [split, stage, jj, wave]
    acc = np.zeros((ksplit, 4, T * Cin, Cout), F32)
    for st in range(stages):
        for jj in range(4):
            acc = (acc.astype(F64) + pairs[:, st, jj]).astype(F32)
    rows = np.zeros((ksplit, T * Cin, Cout), F32)
    for w in range(4):
        rows = (rows + acc[:, w]).astype(F32)
    out = rowsum32(rows).reshape(k, k, Cin, Cout).transpose(3, 2, 0, 1)
    return out if init is None else (np.asarray(init, F32) + out).astype(F32)
