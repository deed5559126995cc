"""References of the zoo's normalisation, element-wise, resampling and concatenation kernels (evf_norm.hip, the tail of
evf_neuron_gen.hip), shared by tests/test_host_zoo_ops_reference.py (CPU) and tests/test_gpu_zoo_ops.py.  Not a test module.

Every FAMILY is one entry point (or one chain of them).  For a family: CASES[family] lists its cases, make(family, case) gives the
seeded float32 inputs, run(family, case, inputs, dtype, mut) evaluates the operation in numpy -- dtype float64 is the reference,
dtype float32 the emulation (every numpy float32 operation rounds once, as the kernels do: the library is built with
-ffp-contract=off) and `mut` one of MUTANTS, a deliberately wrong variant -- and expect(family, case, inputs) turns the float64
result into the assertion of the GPU test, one Out per output:

rule 1  bit for bit.  Data movement, a single correctly rounded operation (float64 rounded to float32 equals the float32
        operation: 53 >= 2 * 24 + 2 bits), and everything fed integer-valued / dyadic inputs whose products and partial sums fit
        in 24 bits, where any association gives the same bits.
rule 2  |got - ref| <= k * 2^-24 * scale, scale = the sum of the |terms| of the output's expression, k = the number of rounded
        operations of the expression (+ the number of summed terms of a reduction).  K2 states k per output.
rule 3  (tanhf / expf / sqrtf / divide)  |got - ref| <= 4 * MEASURED[key] * 2^-24 * scale.  MEASURED is the largest error of the
        float32 emulation against float64 on these very inputs, found by tests/test_host_zoo_ops_reference.py on the CPU and
        stored here; nothing is measured on the kernels.  The factor 4 is the one of tests/step_tail_ref.py: one ulp each for
        the device's functions plus another association.

fractions(expected, got) -> {output: error / bound} (0 or inf under rule 1) is the ONE judgement both test modules use: the GPU
test feeds it the kernels' outputs, the host test the emulation's (must pass) and every mutant's (must fail somewhere)."""

import functools
import itertools

import numpy as np

import zoo_det_ref as ZD

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126  # the smallest normal float32
SENTINEL = -724625.0  # gpu_bufs.SENTINEL: what pre-fills outputs and the padding columns an entry point must not touch

MUTANTS = ("affine_bc_cc_swapped", "wn_bwd_nrm_squared", "gru_h_minus_o", "gru_gh_stored", "lstm_chunk_order",
           "bilinear_align_corners", "up2_bwd_no_border_taps", "concat_off_by_one_part", "vector_path_aligned_down",
           "reduction_drops_tail")

# rule 3: the emulation's largest error, units of 2^-24 * scale (printed and checked by the host test)
MEASURED = {
    "wn_fwd.nrm": 1.35, "wn_fwd.w": 3.09, "wn_bwd.gv": 1.93, "wn_bwd.gg": 1.29,
    "act_fwd.tanh": 1.18, "act_fwd.sigmoid": 1.41,
    "gru_gates_fwd.u": 1.31, "gru_gates_fwd.r": 1.41, "gru_gates_fwd.hr": 1.75, "gru_out_fwd.o": 0.987, "gru_out_fwd.hn": 2.18,
    "gru_chain.g_cu": 0.974, "gru_chain.g_cr": 0.257, "gru_chain.g_co": 1.48, "gru_chain.g_h": 1.61, "gru_chain.hn": 4.17,
    "lstm_fwd.gates": 1.44, "lstm_fwd.cell": 3.98, "lstm_fwd.hidden": 3.96, "lstm_bwd.g_gates": 3.19, "lstm_bwd.g_prev_cell": 2.83,
    "spike_bwd.arctan": 1.81, "spike_bwd.superspike": 1.54, "spike_bwd.multigauss": 2.68,
}
# rule 2: rounded operations per output (a reduction adds its number of terms, see expect())
K2 = {
    "chan_reduce": ZD.CHAN_OPS,  # + npg:  x | (x - c)^2 | y * ((x - c) * s)
    "chan_affine": 4,  # Bc * x, + Cc, A * g, +
    "act_bwd.tanh": 3, "act_bwd.sigmoid": 3,  # o * o, 1 -, gy *   |   1 - o, o *, gy *
    "gru_out_bwd.g_co": 4, "gru_out_bwd.g_cu": 5, "gru_out_bwd.g_h": 2,
    "gru_gates_bwd.g_cr": 4, "gru_gates_bwd.g_h": 2,  # g * h, * r, 1 - r, *   |   g * r, + onto g_h
    "spike_bwd.triangle": 3,  # w * |x|, 1 -, g *
}


class Out:
    """One expected output: ref (float64), the rule, and for rules 2 / 3 the scale [same shape] with k or the MEASURED key."""

    def __init__(self, ref, rule=1, scale=None, k=None, key=None, zero_sign_free=False, table=None):
        self.ref, self.rule, self.scale, self.k, self.key, self.zero_sign_free = np.asarray(ref, F64), rule, scale, k, key, zero_sign_free
        self.table = MEASURED if table is None else table  # (tests/metrics_ref.py keeps its own)

    def factor(self):
        return self.k if self.rule == 2 else 4.0 * self.table[self.key]

    def bound(self):
        """A rounded operation errs by 2^-24 of its result -- or, below the smallest normal number, by up to that number (a
        subnormal result has fewer digits, and may be flushed to zero): TINY per unit on top."""
        return self.factor() * (U * np.asarray(self.scale, F64) + TINY)


def bits_equal(got, ref64, zero_sign_free=False):
    ref = np.asarray(ref64, F64)
    r32 = ref.astype(F32)
    fin = np.isfinite(ref)
    assert np.array_equal(ref[fin], r32.astype(F64)[fin]), "the reference is not exact in float32"
    g32 = np.asarray(got, F32).reshape(r32.shape)
    if zero_sign_free:
        g32, r32 = g32 + F32(0), r32 + F32(0)
    return (g32.view(np.int32) == r32.view(np.int32)) | (np.isnan(g32) & np.isnan(r32))


def fractions(expected, got):
    """{output: largest error / bound}; rule 1: 0.0 or inf.  NaNs must sit where the reference has them."""
    fr = {}
    for name, o in expected.items():
        g = np.asarray(got[name], F64).reshape(-1)
        r = o.ref.reshape(-1)
        assert g.size == r.size, (name, g.size, r.size)
        if o.rule == 1:
            fr[name] = 0.0 if bits_equal(got[name], o.ref, o.zero_sign_free).all() else np.inf
            continue
        if not np.array_equal(np.isnan(g), np.isnan(r)):
            fr[name] = np.inf
            continue
        keep = ~np.isnan(r)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(g == r, 0.0, np.abs(g - r))[keep]
            f = np.where(err == 0.0, 0.0, err / o.bound().reshape(-1)[keep])
        fr[name] = float(np.max(f, initial=0.0))
    return fr


def r32(a):
    """float64 -> the nearest float32, as float64: what ONE correctly rounded float32 operation on float32 operands gives."""
    return np.asarray(a, F64).astype(F32).astype(F64)


def cdiv(a, b):
    return -(-a // b)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _ints(rng, shape, m=64):
    return rng.integers(-m, m + 1, shape).astype(F32)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _c(v, dt):
    return None if v is None else np.asarray(v, dt)


# =========================================================================================================== the sigmoid / tanh
def _sig(v):
    """1 / (1 + exp(-v)) in v's dtype, the kernels' expression."""
    one = v.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-v))


# ============================================================================================================== chan_reduce
# zoo_det_ref's table, plus one pixel / the first size with two blocks per group at 64 channel lanes (npl = 4: 33 > 4 * 8) / the
# first with two blocks at one channel lane (npl = 256: 2049 > 256 * 8)
CHAN_CASES = [(G, npg, C) for C in ZD.CHAN_C for npg in ZD.CHAN_NPG for G in ZD.CHAN_G] + \
             [(G, npg, C) for C in (1, 2, 64, 65, 130) for npg in (1, 33, 2049) for G in (1, 3)]
CHAN_PADS = (0, 3)


def chan_int_inputs(G, npg, C, pad):
    """Integer x in [-8, 8], y in [-4, 4], center in [-2, 2], scale in {1/2, 1, 2}: every term is a multiple of 1/2 of magnitude
    <= 80, every partial sum of <= 40000 terms below 2^23 / 2: exact in float32 in any order."""
    rng = _rng(41, G, npg, C, pad)
    ld = C + pad
    x = np.full((G * npg, ld), 1e6, F32)
    y = np.full((G * npg, ld), 1e6, F32)
    x[:, :C] = rng.integers(-8, 9, (G * npg, C))
    y[:, :C] = rng.integers(-4, 5, (G * npg, C))
    center = rng.integers(-2, 3, (G, C)).astype(F32)
    scale = np.asarray([0.5, 1.0, 2.0], F32)[rng.integers(0, 3, (G, C))]
    return x, y, center, scale


def chan_drop_tail(x, y, G, npg, C):
    """MUTANT reduction_drops_tail: the last npg % (pixel lanes) pixels of every group are not summed."""
    npl = ZD.chan_geometry(G, npg, C)["npl"]
    keep = npg - npg % npl
    x, y = x.copy().reshape(G, npg, -1), y.copy().reshape(G, npg, -1)
    x[:, keep:], y[:, keep:] = 0.0, 0.0  # (a term of mode 1 still holds center^2: different, which is all a mutant must be)
    return x.reshape(G * npg, -1), y.reshape(G * npg, -1)


# =============================================================================================================== chan_affine
AFFINE_CASES = [(G, npg, C, bwd) for G in (1, 3) for npg in (1, 7, 257) for C in (1, 3, 32, 65) for bwd in (0, 1)]


def _make_chan_affine(case):
    G, npg, C, bwd = case
    rng = _rng(43, *case)
    ldg, ldx, ldo = C + 2, C + 5, C + 3
    x = np.full((G * npg, ldx), 1e6, F32)
    g = np.full((G * npg, ldg), 1e6, F32)
    x[:, :C] = rng.normal(0.3, 1.0, (G * npg, C))
    g[:, :C] = rng.normal(0.0, 1.0, (G * npg, C))
    co = lambda: rng.normal(0.0, 1.0, (G, C)).astype(F32)  # noqa: E731
    return {"x": x, "g": g if bwd else None, "A": co(), "Bc": co(), "Cc": co(), "ldg": ldg, "ldx": ldx, "ldo": ldo}


def _run_chan_affine(case, i, dt, mut):
    G, npg, C, bwd = case
    Bc, Cc = (i["Cc"], i["Bc"]) if mut == "affine_bc_cc_swapped" else (i["Bc"], i["Cc"])
    rep = lambda a: np.repeat(_c(a, dt), npg, axis=0)  # noqa: E731  [G, C] -> [G * npg, C]
    x = _c(i["x"][:, :C], dt)
    t1 = rep(Bc) * x
    v = t1 + rep(Cc)
    scale = np.abs(t1) + np.abs(rep(Cc))
    if bwd:
        t2 = rep(i["A"]) * _c(i["g"][:, :C], dt)
        v = v + t2
        scale = scale + np.abs(t2)
    out = np.full((G * npg, i["ldo"]), SENTINEL, dt)
    out[:, :C] = v
    sc = np.ones((G * npg, i["ldo"]), F64)
    sc[:, :C] = scale
    return {"out": out, "_scale": sc}


# =============================================================================================================== weight norm
WN_CASES = [(Cout, n) for Cout in (1, 3, 32) for n in (1, 2, 63, 64, 255, 256, 257, 4608)]
WN_TINY, WN_HUGE = 1e-18, 1e18
FLT_MAX = float(np.finfo(F32).max)


def _make_wn(case):
    """Rows of |v| in [0.5, 1.5].  From Cout = 3 on, row 1 is scaled by 1e-18 and row 2 by 1e+18: the squares of the first stay
    normal float32 numbers (1e-36), the sum of squares of the second overflows float32 once n * 1.08e36 > 3.4e38."""
    Cout, n = case
    rng = _rng(47, Cout, n)
    v = (rng.uniform(0.5, 1.5, (Cout, n)) * rng.choice([-1.0, 1.0], (Cout, n))).astype(F32)
    if Cout >= 3:
        v[1] *= F32(WN_TINY)
        v[2] *= F32(WN_HUGE)
    g = rng.uniform(0.5, 2.0, Cout).astype(F32)
    gw = rng.normal(0, 1, (Cout, n)).astype(F32)
    return {"v": v, "g": g, "gw": gw}


def block_sum32(terms, threads=256):
    """Row sums of [rows, n] as a block of `threads` does in `terms`' dtype: a strided loop per thread, the xor butterfly of a
    wave of 64, the waves in index order."""
    rows, n = terms.shape
    trips = cdiv(n, threads)
    t = np.zeros((rows, trips * threads), terms.dtype)
    t[:, :n] = terms
    t = t.reshape(rows, trips, threads)
    acc = np.zeros((rows, threads), terms.dtype)
    for j in range(trips):
        acc = acc + t[:, j]
    w = acc.reshape(rows, threads // 64, 64)
    lane = np.arange(64)
    o = 32
    while o:
        w = w + w[:, :, lane ^ o]
        o >>= 1
    s = np.zeros(rows, terms.dtype)
    for k in range(threads // 64):
        s = s + w[:, k, 0]
    return s


def wn_overflows(v):
    """Per row: the float64 sum of squares is beyond float32.  The host test asserts a 10 % margin either side."""
    return (np.asarray(v, F64) ** 2).sum(1) > FLT_MAX


def _run_wn_fwd(case, i, dt, mut):
    v, g = _c(i["v"], dt), _c(i["g"], dt)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nrm = np.sqrt(block_sum32(v * v))
        w = v * (g / nrm)[:, None]
    return {"w": w, "nrm": nrm}


def _run_wn_bwd(case, i, dt, mut):
    """nrm: the float32 norms the forward kernel leaves are an INPUT of the backward (the emulation's, for both dtypes)."""
    v, g, gw = _c(i["v"], dt), _c(i["g"], dt), _c(i["gw"], dt)
    nr = _c(i["nrm"], dt)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        dot = block_sum32(gw * v)
        a = g / nr
        # d v = (g / nrm) (gw - v <gw, v> / nrm^2), the form of ATen's weight_norm backward: nrm^2 stays a normal float32 number
        # wherever nrm is one (nrm^3 under- or overflows for rows of magnitude 1e-18 / 1e+18).  MUTANT: one power of nrm short.
        q = dot / (nr if mut == "wn_bwd_nrm_squared" else nr * nr)
        gv = a[:, None] * (gw - v * q[:, None])
        adot = np.abs(gw * v).sum(1)
        sgv = np.abs(a)[:, None] * (np.abs(gw) + np.abs(v) * (adot / (nr * nr))[:, None])
        return {"gv": gv, "gg": dot / nr, "_sgv": sgv, "_sgg": adot / nr}


# =============================================================================================================== element-wise
NS = (1, 255, 256, 257)
SPECIALS = (0.0, -0.0, 88.0, -88.0, 1e-8, -1e-8)
ACT_CASES = [(kind, res, n) for kind in range(4) for res in (0, 1) for n in NS]
ACT_NAMES = {1: "tanh", 2: "sigmoid"}


def _with_specials(rng, n, sd=2.0):
    x = rng.normal(0, sd, n).astype(F32)
    k = min(n, len(SPECIALS))
    x[:k] = SPECIALS[:k]
    return x


def _make_act(case):
    kind, res, n = case
    rng = _rng(53, n)
    r = rng.normal(0, 1, n).astype(F32)
    r[:len(SPECIALS)] = 0.0  # (the special values reach the activation with a residual too)
    return {"x": _with_specials(rng, n), "r": r if res else None, "gy": rng.normal(0, 1, n).astype(F32)}


def _act(kind, v):
    if kind == 1:
        return np.tanh(v)
    if kind == 2:
        return _sig(v)
    if kind == 3:
        return np.maximum(v, v.dtype.type(0))
    return v


def _run_act_fwd(case, i, dt, mut):
    kind, res, n = case
    v = _c(i["x"], dt)
    if res:
        v = v + _c(i["r"], dt)
    return {"y": _act(kind, v)}


def _run_act_bwd(case, i, dt, mut):
    """y: the float32 output of the forward's emulation (an input here, for both dtypes)."""
    kind, res, n = case
    o, gy = _c(i["y"], dt), _c(i["gy"], dt)
    one = dt(1)
    if kind == 1:
        return {"gx": gy * (one - o * o), "_s": np.abs(gy) * (1 + o * o)}
    if kind == 2:
        return {"gx": gy * (o * (one - o)), "_s": np.abs(gy) * np.abs(o) * (1 + np.abs(o))}
    if kind == 3:
        return {"gx": gy * (o > 0).astype(dt)}
    return {"gx": gy * one}


GRU_CASES = [(n, has_h) for n in NS for has_h in (0, 1)]


def _make_gru(case):
    n, has_h = case
    rng = _rng(59, n, has_h)
    u01 = lambda: rng.uniform(0.02, 0.98, n).astype(F32)  # noqa: E731
    return {"cu": _with_specials(rng, n), "cr": _with_specials(rng, n)[::-1].copy(), "co": _with_specials(rng, n, 1.0),
            "h": rng.normal(0, 1, n).astype(F32) if has_h else None, "u": u01(), "r": u01(), "o": rng.uniform(-0.98, 0.98, n).astype(F32),
            "g_new": rng.normal(0, 1, n).astype(F32), "g_hr": rng.normal(0, 1, n).astype(F32), "g_h0": rng.normal(0, 1, n).astype(F32),
            "kk": rng.uniform(-2, 2, n).astype(F32), "c0": rng.normal(0, 1, n).astype(F32)}


def _h(i, dt, n):
    return np.zeros(n, dt) if i["h"] is None else _c(i["h"], dt)


def _run_gru_gates_fwd(case, i, dt, mut):
    h = _h(i, dt, case[0])
    r = _sig(_c(i["cr"], dt))
    return {"u": _sig(_c(i["cu"], dt)), "r": r, "hr": h * r, "_shr": np.abs(h)}


def _run_gru_out_fwd(case, i, dt, mut):
    h, u = _h(i, dt, case[0]), _c(i["u"], dt)
    o = np.tanh(_c(i["co"], dt))
    return {"o": o, "hn": h * (dt(1) - u) + o * u, "_shn": np.abs(h) * (1 + np.abs(u)) + np.abs(o * u)}


def _run_gru_out_bwd(case, i, dt, mut):
    h, u, o, g = _h(i, dt, case[0]), _c(i["u"], dt), _c(i["o"], dt), _c(i["g_new"], dt)
    one = dt(1)
    d = (h - o) if mut == "gru_h_minus_o" else (o - h)
    return {"g_co": g * u * (one - o * o), "g_cu": g * d * u * (one - u), "g_h": g * (one - u),
            "_sg_co": np.abs(g * u) * (1 + o * o), "_sg_cu": np.abs(g) * (np.abs(o) + np.abs(h)) * np.abs(u) * (1 + np.abs(u)),
            "_sg_h": np.abs(g) * (1 + np.abs(u))}


def _run_gru_gates_bwd(case, i, dt, mut):
    h, r, g, gh0 = _h(i, dt, case[0]), _c(i["r"], dt), _c(i["g_hr"], dt), _c(i["g_h0"], dt)
    t = g * r
    return {"g_cr": g * h * r * (dt(1) - r), "g_h": t if mut == "gru_gh_stored" else gh0 + t,
            "_sg_cr": np.abs(g * h * r) * (1 + np.abs(r)), "_sg_h": np.abs(gh0) + np.abs(t)}


def _run_gru_chain(case, i, dt, mut):
    """The four entry points in the order of a step, the out-gate convolution replaced by co = c0 + kk * hr (submodules.py:412-416:
    u, r = sigmoid; o = tanh(conv(cat(x, h * r))); new = h (1 - u) + o u), then the backward of sum(g_new * new)."""
    n = case[0]
    a = _run_gru_gates_fwd(case, i, dt, mut)
    co = _c(i["c0"], dt) + _c(i["kk"], dt) * a["hr"]
    b = _run_gru_out_fwd(case, dict(i, co=co, u=a["u"]), dt, mut)
    c = _run_gru_out_bwd(case, dict(i, u=a["u"], o=b["o"]), dt, mut)
    g_hr = _c(i["kk"], dt) * c["g_co"]
    d = _run_gru_gates_bwd(case, dict(i, r=a["r"], g_hr=g_hr, g_h0=c["g_h"]), dt, mut)
    s = 1 + np.abs(_c(i["kk"], dt)) * (1 + np.abs(_h(i, dt, n)))  # every gradient is a sum of O(|g_new|) terms times these factors
    sg = np.abs(_c(i["g_new"], dt)) * s
    return {"hn": b["hn"], "g_co": c["g_co"], "g_cu": c["g_cu"], "g_cr": d["g_cr"], "g_h": d["g_h"], "co": co, "g_hr": g_hr,
            "_shn": b["_shn"], "_sg": sg}


LSTM_CASES = [(Ch, npix, pc, miss) for Ch in (1, 3, 32) for npix in (1, 7, 257) for pc in (0, 1)
              for miss in ("none", "g_hidden", "g_cell", "g_prev_cell")]
LSTM_ORDER = (0, 1, 2, 3)  # chunks of the gates tensor: in | remember | out | cell


def _make_lstm(case):
    Ch, npix, pc, miss = case
    rng = _rng(61, Ch, npix, pc)
    gates = rng.normal(0, 1.5, (npix, 4 * Ch)).astype(F32)
    k = min(gates.size, len(SPECIALS))
    gates.reshape(-1)[:k] = SPECIALS[:k]
    f = lambda: rng.normal(0, 1, (npix, Ch)).astype(F32)  # noqa: E731
    return {"gates": gates, "prev_cell": f() if pc else None, "g_hidden": None if miss == "g_hidden" else f(),
            "g_cell": None if miss == "g_cell" else f()}


def _run_lstm_fwd(case, i, dt, mut):
    Ch, npix = case[0], case[1]
    g = _c(i["gates"], dt).reshape(npix, 4, Ch)
    order = (0, 2, 1, 3) if mut == "lstm_chunk_order" else LSTM_ORDER  # MUTANT: `out` and `remember` trade places
    ig, rg, og, cg = _sig(g[:, order[0]]), _sig(g[:, order[1]]), _sig(g[:, order[2]]), np.tanh(g[:, order[3]])
    pc = np.zeros((npix, Ch), dt) if i["prev_cell"] is None else _c(i["prev_cell"], dt)
    cn = rg * pc + ig * cg
    act = np.empty((npix, 4, Ch), dt)
    act[:, order[0]], act[:, order[1]], act[:, order[2]], act[:, order[3]] = ig, rg, og, cg
    return {"gates": act.reshape(npix, 4 * Ch), "cell": cn, "hidden": og * np.tanh(cn), "_scell": np.abs(rg * pc) + np.abs(ig * cg),
            "_shidden": np.abs(og)}


def _run_lstm_bwd(case, i, dt, mut):
    """act / cell: the float32 outputs of the forward's emulation (inputs here, for both dtypes)."""
    Ch, npix = case[0], case[1]
    a = _c(i["act"], dt).reshape(npix, 4, Ch)
    ig, rg, og, cg = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    z = np.zeros((npix, Ch), dt)
    tc = np.tanh(_c(i["cell"], dt))
    gh = z if i["g_hidden"] is None else _c(i["g_hidden"], dt)
    gcell = z if i["g_cell"] is None else _c(i["g_cell"], dt)
    pc = z if i["prev_cell"] is None else _c(i["prev_cell"], dt)
    one = dt(1)
    gc = gcell + gh * og * (one - tc * tc)
    sgc = np.abs(gcell) + np.abs(gh * og) * (1 + tc * tc)
    go = np.stack([gc * cg * ig * (one - ig), gc * pc * rg * (one - rg), gh * tc * og * (one - og), gc * ig * (one - cg * cg)], 1)
    sgo = np.stack([sgc * np.abs(cg * ig) * (1 + np.abs(ig)), sgc * np.abs(pc * rg) * (1 + np.abs(rg)),
                    np.abs(gh * tc * og) * (1 + np.abs(og)), sgc * np.abs(ig) * (1 + cg * cg)], 1)
    return {"g_gates": go.reshape(npix, 4 * Ch), "g_prev_cell": gc * rg, "_sg_gates": sgo.reshape(npix, 4 * Ch),
            "_sg_prev_cell": sgc * np.abs(rg)}


SURROGATES = {0: "arctan", 1: "superspike", 2: "triangle", 3: "multigauss"}
SPIKE_WIDTH = {0: 10.0, 1: 10.0, 2: 1.0, 3: 0.5}
SPIKE_CASES = [(s, per, n) for s in range(4) for per in (0, 1) for n in NS]


def _make_spike(case):
    """x at exactly the threshold and one ulp either side (elements 0 - 2 of every block of 8), else within +- 2 of it."""
    s, per, n = case
    rng = _rng(67, per, n)
    th = rng.uniform(0.5, 1.5, n).astype(F32) if per else np.asarray([0.75], F32)
    t = np.broadcast_to(th, (n,))
    x = (t + rng.uniform(-2, 2, n)).astype(F32)
    idx = np.arange(n)
    x = np.where(idx % 8 == 0, t, x)
    x = np.where(idx % 8 == 1, np.nextafter(t, F32(np.inf)), x)
    x = np.where(idx % 8 == 2, np.nextafter(t, F32(-np.inf)), x)
    return {"x": x.astype(F32), "th": th, "g": rng.normal(0, 1, n).astype(F32)}


def _run_spike_fwd(case, i, dt, mut):
    return {"z": ((_c(i["x"], dt) - _c(i["th"], dt)) > 0).astype(dt)}


def _run_spike_bwd(case, i, dt, mut):
    s = case[0]
    w = dt(F32(SPIKE_WIDTH[s]))
    x, g = _c(i["x"], dt) - _c(i["th"], dt), _c(i["g"], dt)
    one = dt(1)
    if s == 1:
        d = one + w * np.abs(x)
        sg = one / (d * d)
    elif s == 2:
        sg = np.maximum(dt(0), one - w * np.abs(x))
    elif s == 3:
        s1, s2, k = w, dt(6) * w, dt(F32(0.3989422804014327))
        gs = lambda v, mu, sd: np.exp(-((v - mu) * (v - mu)) / (dt(2) * sd * sd)) / sd * k  # noqa: E731
        sg = dt(F32(1.15)) * gs(x, dt(0), s1) - dt(F32(0.15)) * gs(x, w, s2) - dt(F32(0.15)) * gs(x, -w, s2)
    else:
        sg = one / (one + w * x * x)
    if s == 2:
        scale = np.abs(g) * (1 + w * np.abs(x))
    elif s == 3:  # (the three Gaussians' magnitudes: the difference cancels)
        scale = np.abs(g) * 0.3989422804014327 * (1.15 / float(w) + 0.3 / (6.0 * float(w)))
    else:
        scale = np.abs(g)
    return {"gx": g * sg, "_s": scale}


# ================================================================================================================ resampling
UP2_HW = ((1, 1), (1, 5), (4, 1), (2, 2), (5, 7))
UP2_CASES = [(B, H, W, C, shift) for (H, W) in UP2_HW for C in (1, 2, 3, 4, 6, 8) for shift in (0, 1, 2) for B in (1, 2)]


def up2_matrix(n, mut=None):
    """[2n, n] float64: the 1-D bilinear x2 operator, align_corners False, source index clamped (ATen's area_pixel_compute)."""
    M = np.zeros((2 * n, n), F64)
    for o in range(2 * n):
        if mut == "bilinear_align_corners":
            s = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
        else:
            s = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = int(s)
        clamped = i0 >= n - 1
        i1 = i0 + (0 if clamped else 1)
        w1 = s - i0
        M[o, i0] += 1.0 - w1
        if not (clamped and mut == "up2_bwd_no_border_taps"):  # MUTANT: the tap that the clamp folds onto the border pixel is lost
            M[o, i1] += w1
    return M


def _make_up2(case):
    B, H, W, C, shift = case
    rng = _rng(71, B, H, W, C)
    return {"x": _ints(rng, (B, H, W, C)), "gy": _ints(rng, (B, 2 * H, 2 * W, C))}


def _aligned_down(a, shift):
    """MUTANT vector_path_aligned_down: the vector kernel runs on the pointer rounded down to its vector: every load sees the
    floats `shift` places before its own (the first ones the guard in front of the buffer)."""
    flat = np.concatenate([np.full(shift, SENTINEL, a.dtype), a.reshape(-1)])[:a.size]
    return flat.reshape(a.shape)


def _up2_vec_mutant(case, a, mut):
    C, shift = case[3], case[4]
    if mut != "vector_path_aligned_down":
        return a
    if C % 4 == 0 and shift % 4:
        return _aligned_down(a, shift % 4)
    return _aligned_down(a, 1) if (C % 2 == 0 and shift % 2) else a


def _run_up2_fwd(case, i, dt, mut):
    B, H, W, C, shift = case
    m = mut if mut == "bilinear_align_corners" else None
    x = _up2_vec_mutant(case, _c(i["x"], dt), mut)
    return {"y": np.einsum("oh,pw,bhwc->bopc", up2_matrix(H, m).astype(dt), up2_matrix(W, m).astype(dt), x) + dt(0)}


def _run_up2_bwd(case, i, dt, mut):
    B, H, W, C, shift = case
    m = mut if mut == "up2_bwd_no_border_taps" else None
    gy = _up2_vec_mutant(case, _c(i["gy"], dt), mut)
    return {"gx": np.einsum("oh,pw,bopc->bhwc", up2_matrix(H, m).astype(dt), up2_matrix(W, m).astype(dt), gy) + dt(0)}


NEAR_CASES = [(planes, h, w, f) for f in (1, 2, 4) for planes in (1, 3) for (h, w) in ((1, 1), (3, 5))]


def _make_near(case):
    planes, h, w, f = case
    rng = _rng(73, *case)
    return {"x": rng.normal(0, 1, (planes, h, w)).astype(F32), "gy": _ints(rng, (planes, h * f, w * f))}


def _run_near_fwd(case, i, dt, mut):
    f = case[3]
    return {"y": np.repeat(np.repeat(_c(i["x"], dt), f, axis=1), f, axis=2)}


def _run_near_bwd(case, i, dt, mut):
    planes, h, w, f = case
    return {"gx": _c(i["gy"], dt).reshape(planes, h, f, w, f).sum((2, 4)) + dt(0)}


# (channels of the parts (None: a null part = zeros of that many channels), extra stride of every part, extra stride of out)
CONCAT_CASES = [(((5, 1),), 0, 0), (((5, 1),), 2, 3), (((3, 1), (4, 1), (1, 1)), 1, 2), (((2, 1), (7, 0), (3, 1)), 3, 1),
                (((2, 1), (3, 1), (2, 0)), 0, 5), (((1, 1), (3, 1), (2, 0), (5, 1), (7, 1), (1, 0)), 2, 3)]
CONCAT_NPIX = (1, 37, 300)


def _parts(rng, chans, npix, pad, ints):
    parts = []
    for k, (Ck, present) in enumerate(chans):
        if not present:
            parts.append(None)
            continue
        a = np.full((npix, Ck + pad + (2 * k if pad else 0)), 1e6, F32)  # (every part its own stride)
        a[:, :Ck] = _ints(rng, (npix, Ck)) if ints else rng.normal(0, 1, (npix, Ck))
        parts.append(a)
    return parts


def _concat(chans, parts, npix, dt, mut):
    n = len(chans)
    cols = []
    for k, (Ck, present) in enumerate(chans):
        j = (k + 1) % n if (mut == "concat_off_by_one_part" and n > 1) else k  # MUTANT: channel block k reads the next part
        src = parts[j]
        if src is None:
            cols.append(np.zeros((npix, Ck), dt))
        else:
            take = np.arange(Ck) % chans[j][0]
            cols.append(np.asarray(src, dt)[:, take])
    return np.concatenate(cols, 1)


def _make_concat(case):
    (chans, pad, opad), npix = case
    return {"parts": _parts(_rng(79, len(chans), pad, npix), chans, npix, pad, ints=False)}


def _run_concat(case, i, dt, mut):
    (chans, pad, opad), npix = case
    cat = _concat(chans, i["parts"], npix, dt, mut)
    out = np.full((npix, cat.shape[1] + opad), SENTINEL, dt)
    out[:, :cat.shape[1]] = cat
    return {"out": out}


# parts of evf_concat_up2_fwd: a channel quad that straddles two parts (2 | 16: channels 0-1 and 2-3), a part and the zero
# padding (.. | 16 | null 2), and (6 | 2 | null 4): quad 1 = part 0's last pair + part 1, quad 2 = padding alone
CUP_PARTS = (((2, 1), (16, 1), (16, 1), (2, 0)), ((2, 1), (2, 1)), ((6, 1), (2, 1), (4, 0)))
CUP_CASES = [(chans, B, H, W, pad) for chans in CUP_PARTS for (H, W) in ((1, 1), (1, 4), (3, 1), (5, 7)) for B, pad in ((1, 0), (2, 2))]


def _make_cup(case):
    chans, B, H, W, pad = case
    return {"parts": _parts(_rng(83, len(chans), B, H, W, pad), chans, B * H * W, pad, ints=True)}


def _run_cup(case, i, dt, mut):
    chans, B, H, W, pad = case
    cat = _concat(chans, i["parts"], B * H * W, dt, mut).reshape(B, H, W, -1)
    y = _run_up2_fwd((B, H, W, cat.shape[-1], 0), {"x": cat}, dt, mut)["y"]
    out = np.full((B, 2 * H, 2 * W, cat.shape[-1] + 4), SENTINEL, dt)
    out[..., :cat.shape[-1]] = y
    return {"out": out}


# ================================================================================================================== the table
CASES = {
    "chan_affine": AFFINE_CASES, "wn_fwd": WN_CASES, "wn_bwd": WN_CASES, "act_fwd": ACT_CASES, "act_bwd": ACT_CASES,
    "gru_gates_fwd": GRU_CASES, "gru_out_fwd": GRU_CASES, "gru_out_bwd": GRU_CASES, "gru_gates_bwd": GRU_CASES, "gru_chain": GRU_CASES,
    "lstm_fwd": [c for c in LSTM_CASES if c[3] == "none"], "lstm_bwd": LSTM_CASES, "spike_fwd": [c for c in SPIKE_CASES if c[0] == 0],
    "spike_bwd": SPIKE_CASES, "up2_fwd": UP2_CASES, "up2_bwd": UP2_CASES, "near_fwd": NEAR_CASES, "near_bwd": NEAR_CASES,
    "concat": list(itertools.product(CONCAT_CASES, CONCAT_NPIX)), "concat_up2": CUP_CASES,
}
_MAKE = {"chan_affine": _make_chan_affine, "wn_fwd": _make_wn, "wn_bwd": _make_wn, "act_fwd": _make_act, "act_bwd": _make_act,
         "gru_gates_fwd": _make_gru, "gru_out_fwd": _make_gru, "gru_out_bwd": _make_gru, "gru_gates_bwd": _make_gru,
         "gru_chain": _make_gru, "lstm_fwd": _make_lstm, "lstm_bwd": _make_lstm, "spike_fwd": _make_spike, "spike_bwd": _make_spike,
         "up2_fwd": _make_up2, "up2_bwd": _make_up2, "near_fwd": _make_near, "near_bwd": _make_near, "concat": _make_concat,
         "concat_up2": _make_cup}
_RUN = {"chan_affine": _run_chan_affine, "wn_fwd": _run_wn_fwd, "wn_bwd": _run_wn_bwd, "act_fwd": _run_act_fwd, "act_bwd": _run_act_bwd,
        "gru_gates_fwd": _run_gru_gates_fwd, "gru_out_fwd": _run_gru_out_fwd, "gru_out_bwd": _run_gru_out_bwd,
        "gru_gates_bwd": _run_gru_gates_bwd, "gru_chain": _run_gru_chain, "lstm_fwd": _run_lstm_fwd, "lstm_bwd": _run_lstm_bwd,
        "spike_fwd": _run_spike_fwd, "spike_bwd": _run_spike_bwd, "up2_fwd": _run_up2_fwd, "up2_bwd": _run_up2_bwd,
        "near_fwd": _run_near_fwd, "near_bwd": _run_near_bwd, "concat": _run_concat, "concat_up2": _run_cup}
FAMILIES = tuple(CASES)
# the families on which a mutant acts (the host test looks for its failure there)
MUTANT_FAMILIES = {"affine_bc_cc_swapped": ("chan_affine",), "wn_bwd_nrm_squared": ("wn_bwd",), "gru_h_minus_o": ("gru_out_bwd",),
                   "gru_gh_stored": ("gru_gates_bwd",), "lstm_chunk_order": ("lstm_fwd",),
                   "bilinear_align_corners": ("up2_fwd", "concat_up2"),
                   "up2_bwd_no_border_taps": ("up2_bwd",), "concat_off_by_one_part": ("concat", "concat_up2"),
                   "vector_path_aligned_down": ("up2_fwd", "up2_bwd"), "reduction_drops_tail": ("chan_reduce",)}


@functools.lru_cache(maxsize=None)
def make(family, case):
    """The inputs of a case (read-only, shared).  The backward families get the float32 emulation of their forward as inputs:
    wn_bwd `nrm`, act_bwd `y`, lstm_bwd `act` and `cell`."""
    i = dict(_MAKE[family](case))
    if family == "wn_bwd":
        i["nrm"] = _run_wn_fwd(case, i, F32, None)["nrm"]
    elif family == "act_bwd":
        i["y"] = _run_act_fwd(case, i, F32, None)["y"]
    elif family == "lstm_bwd":
        f = _run_lstm_fwd(case, i, F32, None)
        i["act"], i["cell"] = f["gates"], f["cell"]
    return _freeze(i)


def run(family, case, inputs, dtype=F64, mut=None):
    """{output: array of dtype} (+ the scales of rules 2 / 3 under "_..." keys)."""
    assert mut is None or mut in MUTANTS, mut
    return _RUN[family](case, inputs, dtype, mut)


def outputs(result):
    return {k: v for k, v in result.items() if not k.startswith("_")}


def expect(family, case, inputs):
    """{output: Out}: what the GPU test asserts of this case."""
    r = run(family, case, inputs, F64)
    if family == "chan_affine":
        return {"out": Out(r["out"], 2, r["_scale"], k=K2["chan_affine"])}
    if family == "wn_fwd":
        return _expect_wn_fwd(case, inputs, r)
    if family == "wn_bwd":
        return _expect_wn_bwd(case, inputs, r)
    if family == "act_fwd":
        kind = case[0]
        if kind in ACT_NAMES:
            return {"y": Out(r["y"], 3, np.ones(case[2]), key="act_fwd." + ACT_NAMES[kind])}
        return {"y": Out(r32(r["y"]), 1, zero_sign_free=True)}  # (x + no residual is x + 0: -0 becomes +0; max(-0, +0) has either sign)
    if family == "act_bwd":
        kind = case[0]
        if kind in ACT_NAMES:
            return {"gx": Out(r["gx"], 2, r["_s"], k=K2["act_bwd." + ACT_NAMES[kind]])}
        return {"gx": Out(r["gx"], 1, zero_sign_free=True)}  # (gy * 0: the product's zero carries gy's sign)
    if family == "gru_gates_fwd":
        one = np.ones(case[0])
        return {"u": Out(r["u"], 3, one, key="gru_gates_fwd.u"), "r": Out(r["r"], 3, one, key="gru_gates_fwd.r"),
                "hr": Out(r["hr"], 3, r["_shr"], key="gru_gates_fwd.hr")}
    if family == "gru_out_fwd":
        return {"o": Out(r["o"], 3, np.ones(case[0]), key="gru_out_fwd.o"), "hn": Out(r["hn"], 3, r["_shn"], key="gru_out_fwd.hn")}
    if family in ("gru_out_bwd", "gru_gates_bwd"):
        return {k: Out(v, 2, r["_s" + k], k=K2[f"{family}.{k}"]) for k, v in outputs(r).items()}
    if family == "gru_chain":
        e = {k: Out(r[k], 3, r["_sg"], key="gru_chain." + k) for k in ("g_co", "g_cu", "g_cr", "g_h")}
        e["hn"] = Out(r["hn"], 3, r["_shn"], key="gru_chain.hn")
        return e
    if family == "lstm_fwd":
        return {"gates": Out(r["gates"], 3, np.ones_like(r["gates"]), key="lstm_fwd.gates"),
                "cell": Out(r["cell"], 3, r["_scell"], key="lstm_fwd.cell"),
                "hidden": Out(r["hidden"], 3, r["_shidden"], key="lstm_fwd.hidden")}
    if family == "lstm_bwd":
        e = {"g_gates": Out(r["g_gates"], 3, r["_sg_gates"], key="lstm_bwd.g_gates")}
        if case[3] != "g_prev_cell":
            e["g_prev_cell"] = Out(r["g_prev_cell"], 3, r["_sg_prev_cell"], key="lstm_bwd.g_prev_cell")
        return e
    if family == "spike_bwd":
        name = SURROGATES[case[0]]
        if name == "triangle":
            return {"gx": Out(r["gx"], 2, r["_s"], k=K2["spike_bwd.triangle"])}
        return {"gx": Out(r["gx"], 3, r["_s"], key="spike_bwd." + name)}
    return {k: Out(v, 1) for k, v in outputs(r).items()}  # spike_fwd, up2, nearest, the concatenations


def _expect_wn_fwd(case, inputs, r):
    """Rows whose sum of squares overflows float32: torch's own float32 weight_norm gives nrm = inf and w = v * (g / inf) = 0
    there (tests/test_host_zoo_ops_reference.py shows it), and so does the kernel's expression: parity with torch-float32
    semantics is asserted for them, the float64 reference for every other row (the 1e-18 row included)."""
    ov = wn_overflows(inputs["v"])
    nrm, w = r["nrm"].copy(), r["w"].copy()
    nrm[ov], w[ov] = np.inf, 0.0
    return {"nrm": Out(nrm, 3, np.where(ov, 1.0, r["nrm"]), key="wn_fwd.nrm"),
            "w": Out(w, 3, np.where(ov[:, None], 1.0, np.abs(r["w"])), key="wn_fwd.w")}


def _expect_wn_bwd(case, inputs, r):
    """Overflowed rows (nrm = inf): g / inf = 0 and <gw, v> / inf = 0 (these inputs keep the dot product finite: |gw v| ~ 1e18),
    gv = 0 * (gw - v * 0) = 0, gg = 0: torch's float32 semantics again."""
    ov = wn_overflows(inputs["v"])
    gv, gg = r["gv"].copy(), r["gg"].copy()
    gv[ov], gg[ov] = 0.0, 0.0
    return {"gv": Out(gv, 3, np.where(ov[:, None], 1.0, r["_sgv"]), key="wn_bwd.gv"),
            "gg": Out(gg, 3, np.where(ov, 1.0, r["_sgg"]), key="wn_bwd.gg")}
