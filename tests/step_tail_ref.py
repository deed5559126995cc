"""References for the tail of a training step: clip + Adam (evf_clip_adam_step / evf_clip_adam_fused) and the gradient
collection (evf_grads_finalize, evf_reduce_slabs*, evf_sum_rows, evf_add_segments, evf_unpack_conv_wgrad), in plain numpy.

Shared by tests/test_host_step_tail_reference.py (which establishes the bounds below without a GPU) and
tests/test_gpu_step_tail.py (which holds the kernels to them).  Not a test module itself.

The hyper-parameters cross the C ABI as `float`: every reference here rounds them to fp32 FIRST (b1 = fp32(0.9), ...) and
then works in its own precision, so the fp64 reference and the kernels compute the same function.
"""

import functools

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit round-off of fp32

# the project's values (train.FlatAdam's defaults)
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 2e-4
STEPS = 12

MUTANTS = ("eps_inside_bias_correction", "bias_correction_in_fp32", "coef_without_1e-6", "step_off_by_one",
           "v_from_unclipped_gradient", "norm_skips_the_tail")

# ---- bounds on the normalised errors (units: see normalised_errors) -----------------------------------------------------
# Measured: the worst error of the fp32 emulation adam_ref(dtype=float32) against adam_ref(dtype=float64), teacher-forced,
# over 12 steps x the three clip regimes x n in {5, 1025, 75011} (tests/test_host_step_tail_reference.py prints them):
#     p 5.00   m 0.895   v 0.0482   sumsq 1.06e-7
# Bound = 4 x measured (rounded up to the digits shown).  The factor covers what the emulation does not share with the
# kernels: another summation order for the norm, and one ulp each for the hardware sqrt and divide.
MEASURED = {"p": 5.00, "m": 0.895, "v": 0.0482, "sumsq": 1.06e-7}
BOUND = {k: 4.0 * x for k, x in MEASURED.items()}


# ------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(n, seed=0):
    """-> p [n] fp32, s [n] fp64 (signed per-element gradient scale).
    p: exact zeros (one in eight) plus magnitudes log-uniform over 1e-6 .. 1 with random signs -- an error of the update must not
    hide below the ulp of p.  s: log-uniform over 1e-10 .. 10 with a fixed sign per element: no cancellation in m, and elements
    where eps = 1e-8 dominates sqrt(v_hat).  The LAST element carries the top of the range, so that a sum of squares that drops
    the n % 4 tail shows in the norm at every size."""
    rng = np.random.default_rng(1000 + seed)
    p = 10.0 ** rng.uniform(-6.0, 0.0, n) * rng.choice([-1.0, 1.0], n)
    p[rng.integers(0, 8, n) == 0] = 0.0
    s = 10.0 ** rng.uniform(-10.0, 1.0, n) * rng.choice([-1.0, 1.0], n)
    s[-1] = 10.0
    return p.astype(F32), s


REGIMES = ("none", "above", "clipped")


def regime(name, s):
    """-> (max_norm, gradient scale).  none: no clipping (max_norm 0); above: max_norm far above the norm (coef = 1 through the
    min); clipped: the gradient is scaled to a norm of about 1e-3 and max_norm is 10x below it, so that the +1e-6 of
    clip_grad_norm_ is worth about 1e-3 relative."""
    if name == "none":
        return 0.0, 1.0
    if name == "above":
        return 1e6, 1.0
    assert name == "clipped"
    return 1e-4, 1e-3 / float(np.sqrt(np.sum(s * s)))


def gradient(s, scale, t, seed=0):
    """Gradient of step t (1-based): s_i * (1 + 0.3 u_t,i), u uniform over [-1, 1), times the regime's scale.  Magnitudes are
    kept above 1e-15, so that (1 - b2) (g coef)^2 stays a NORMAL fp32 number in the clipped regime (the bounds are relative)."""
    u = np.random.default_rng(77000 + 131 * seed + t).uniform(-1.0, 1.0, s.shape[0])
    g = s * (1.0 + 0.3 * u) * scale
    g = np.sign(s) * np.maximum(np.abs(g), 1e-15)
    return g.astype(F32)


# -------------------------------------------------------------------------------------------------------------- Adam
def _sumsq_f32(g):
    """Sum of squares in fp32 in the order of k_clip_adam_fused: 1024 threads stride over the float4s with one accumulator per
    component, the n % 4 tail goes to component 0 of the first threads, (s0 + s1) + (s2 + s3), then the block's 1024 sums."""
    n = g.shape[0]
    n4 = n >> 2
    sq = g * g  # fp32
    trips = -(-max(n4, 1) // 1024)
    body = np.zeros(trips * 4096, F32)
    body[: 4 * n4] = sq[: 4 * n4]
    acc = np.add.reduce(body.reshape(trips, 1024, 4), axis=0, dtype=F32) if trips > 1 else body.reshape(1024, 4).copy()
    tail = sq[4 * n4:]
    acc[: tail.shape[0], 0] += tail
    per_thread = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    return np.sum(per_thread, dtype=F32)


def adam_ref(p, g, m, v, *, max_norm, lr=LR, b1=B1, b2=B2, eps=EPS, t, dtype=F64, mutation=None):
    """One step of clip_grad_norm_(max_norm) + torch.optim.Adam as include/evflow.h documents it:
        coef = min(1, max_norm / (|g| + 1e-6))   (1 when max_norm <= 0)
        m' = b1 m + (1 - b1) g coef,   v' = b2 v + (1 - b2) (g coef)^2
        p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    dtype=float64: the reference.  dtype=float32: an emulation in the kernels' operation order (k_clip_adam /
    k_clip_adam_fused; the library is built without FMA contraction); the bias corrections stay in double and are then cast,
    as the kernels do.  mutation: one of MUTANTS, a deliberately wrong variant.  -> p', m', v', sumsq (arrays of `dtype`)."""
    assert mutation is None or mutation in MUTANTS, mutation
    T = dtype
    lr_d, b1_d, b2_d = F64(F32(lr)), F64(F32(b1)), F64(F32(b2))  # what the C ABI hands over
    eps_T, b1_T, b2_T = T(F32(eps)), T(F32(b1)), T(F32(b2))
    p, g, m, v = (np.asarray(a).astype(T) for a in (p, g, m, v))
    n = g.shape[0]
    if T is F32:
        sumsq = _sumsq_f32(g[: n - (n & 3)] if mutation == "norm_skips_the_tail" else g)
    else:
        sumsq = np.sum((g[: n - (n & 3)] if mutation == "norm_skips_the_tail" else g) ** 2, dtype=F64)
    coef = T(1.0)
    if max_norm > 0:
        damp = T(0.0) if mutation == "coef_without_1e-6" else T(1e-6)
        coef = min(T(1.0), T(T(F32(max_norm)) / T(np.sqrt(T(sumsq)) + damp)))
    tt = t + 1 if mutation == "step_off_by_one" else t
    if mutation == "bias_correction_in_fp32":
        step_size = F32(F32(lr) / (F32(1.0) - np.power(F32(b1), F32(tt), dtype=F32)))
        bc2_sqrt = np.sqrt(F32(1.0) - np.power(F32(b2), F32(tt), dtype=F32), dtype=F32)
    else:
        step_size = lr_d / (1.0 - b1_d ** tt)
        bc2_sqrt = np.sqrt(1.0 - b2_d ** tt)
    step_size, bc2_sqrt = T(step_size), T(bc2_sqrt)  # (the cast of the kernels; nothing for the fp64 reference)
    gi = g * coef
    mi = b1_T * m + (T(1.0) - b1_T) * gi
    gv = g if mutation == "v_from_unclipped_gradient" else gi
    vi = b2_T * v + (T(1.0) - b2_T) * gv * gv
    if mutation == "eps_inside_bias_correction":
        denom = (np.sqrt(vi) + eps_T) / bc2_sqrt
    else:
        denom = np.sqrt(vi) / bc2_sqrt + eps_T
    pn = p - step_size * (mi / denom)
    for a in (pn, mi, vi):
        assert a.dtype == T
    return pn, mi, vi, T(sumsq)


def ref_coef(g, max_norm):
    """The fp64 clip coefficient of adam_ref."""
    if max_norm <= 0:
        return 1.0
    return min(1.0, float(F64(F32(max_norm)) / (np.sqrt(np.sum(g.astype(F64) ** 2)) + 1e-6)))


def normalised_errors(got, prev, g, *, max_norm, t, lr=LR, b1=B1, b2=B2, eps=EPS, ref=None):
    """Errors of one step against the fp64 reference that starts from the SAME fp32 state (teacher forcing).
    got = (p', m', v', sumsq) of the code under test, prev = (p, m, v) it started from.  -> {"p", "m", "v", "sumsq"}: the worst
        |m' - m_ref| / (2^-24 (|m_prev| + |g| coef)),   |v' - v_ref| / (2^-24 (v_prev + (g coef)^2)),
        |p' - p_ref| / (2^-24 max(|p_ref|, lr)),        |sumsq - sumsq_ref| / sumsq_ref."""
    p0, m0, v0 = (np.asarray(a).astype(F64) for a in prev)
    if ref is None:  # (ref: the same step by another fp64 implementation, e.g. torch.optim.Adam on the CPU)
        ref = adam_ref(p0, g, m0, v0, max_norm=max_norm, lr=lr, b1=b1, b2=b2, eps=eps, t=t, dtype=F64)
    pr, mr, vr, sr = (np.asarray(a, F64) for a in ref)
    gc = np.abs(g.astype(F64)) * ref_coef(g, max_norm)
    pg, mg, vg, sg = (np.asarray(a).astype(F64) for a in got)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {
            "p": np.max(np.abs(pg - pr) / (U * np.maximum(np.abs(pr), float(F32(lr))))),
            "m": np.max(np.abs(mg - mr) / (U * (np.abs(m0) + gc))),
            "v": np.max(np.abs(vg - vr) / (U * (v0 + gc * gc))),
            "sumsq": abs(float(sg) - float(sr)) / float(sr),
        }
    return {k: (float(x) if np.isfinite(x) else float("inf")) for k, x in out.items()}


@functools.lru_cache(maxsize=8)
def case_inputs(n, regime_name, seed=0):
    """(p0, max_norm, [g_1 .. g_STEPS]) of one (size, clip regime), generated once and shared (read-only) by the tests."""
    p, s = make_inputs(n, seed)
    max_norm, scale = regime(regime_name, s)
    gs = [gradient(s, scale, t, seed) for t in range(1, STEPS + 1)]
    for a in [p] + gs:
        a.setflags(write=False)
    return p, max_norm, gs


def run_emulation(n, regime_name, mutation=None, seed=0):
    """STEPS steps of the fp32 emulation (or a mutant of it) from m = v = 0 -> the worst normalised error per quantity."""
    p, max_norm, gs = case_inputs(n, regime_name, seed)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    worst = dict.fromkeys(("p", "m", "v", "sumsq"), 0.0)
    for t, g in enumerate(gs, 1):
        got = adam_ref(p, g, m, v, max_norm=max_norm, t=t, dtype=F32, mutation=mutation)
        e = normalised_errors(got, (p, m, v), g, max_norm=max_norm, t=t)
        worst = {k: max(worst[k], e[k]) for k in worst}
        p, m, v = got[:3]
    return worst


# ------------------------------------------------------------------------------------------------- gradient collection
NW = 9 * 32 * 32  # elements of a 32 -> 32 3x3 conv weight


def slab_to_torch_layout(x):
    """[9][ci][co] (tap-major, the kernels' slab layout) -> torch's [co][ci][3][3]."""
    return np.ascontiguousarray(np.asarray(x).reshape(9, 32, 32).transpose(2, 1, 0)).reshape(32, 32, 3, 3)


def reduce_slabs_ref(slabs, dst=None):
    """dst [32][32][3][3] (+)= the sum over the slabs [nslab][9*32*32], transposed.  fp64 (exact for the integer-valued tests)."""
    s = slab_to_torch_layout(np.asarray(slabs, F64).reshape(-1, NW).sum(axis=0))
    return s if dst is None else np.asarray(dst, F64).reshape(32, 32, 3, 3) + s


def sum_rows_ref(rows, dst, accumulate):
    """evf_sum_rows: bit 0 of accumulate adds to dst (else overwrites), bit 1 zeroes the rows.  -> dst', rows'."""
    rows = np.asarray(rows, F64)
    s = rows.sum(axis=0)
    return (np.asarray(dst, F64) + s if accumulate & 1 else s), (np.zeros_like(rows) if accumulate & 2 else rows.copy())


def add_segments_ref(src, dsts, off, n, clear):
    """evf_add_segments: dst_k[i] += src[off_k + i], i < n_k; clear: the consumed source elements are zeroed.  -> dsts', src'."""
    src = np.asarray(src, F64)
    out, after = [], src.copy()
    for d, o, k in zip(dsts, off, n):
        d = np.asarray(d, F64).copy()
        d[:k] += src[o:o + k]
        out.append(d)
        if clear:
            after[o:o + k] = 0.0
    return out, after


def finalize_ref(slabs, slab_dst, small, clear_small, rows, head_rows, head_off, seg_dst, seg_off, seg_n, seg_rows=None):
    """The header's contract of evf_grads_finalize in fp64:
        slab_dst[t] += sum of slabs[t] [nslab][9*32*32], transposed to [co][ci][3][3];
        total[e] = small[e] + sum_r rows[r][e] (e < ncols) + sum_r head_rows[r][e - head_off] (head_off <= e < head_off + nhcols);
        seg_dst[k][i] += total[seg_off[k] + i], i < seg_n[k].
    Afterwards: the segments' columns of `rows` are zero in the rows [0, min(nrows, seg_rows[k])) and nothing else of `rows`
    changed; head_rows unchanged; the segments' elements of `small` are zero if clear_small, `small` unchanged otherwise.
    rows / head_rows may be None; seg_rows None or an entry <= 0: all rows.
    -> {"slab_dst": [...], "seg_dst": [...], "small", "rows", "head_rows"} (fp64 arrays, None where the input was None)."""
    out = {"slab_dst": [reduce_slabs_ref(s, d) for s, d in zip(slabs, slab_dst)]}
    small = None if small is None else np.asarray(small, F64)
    rows_after = None if rows is None else np.asarray(rows, F64).copy()
    small_after = None if small is None else small.copy()
    segs = []
    for k, (d, o, n) in enumerate(zip(seg_dst, seg_off, seg_n)):
        e = np.arange(o, o + n)
        total = small[e].copy()
        if rows is not None:
            nrows, ncols = rows_after.shape
            inside = e[e < ncols]
            total[: inside.shape[0]] += np.asarray(rows, F64)[:, inside].sum(axis=0)
            lim = nrows if seg_rows is None or seg_rows[k] <= 0 else min(nrows, seg_rows[k])
            rows_after[:lim, inside] = 0.0
        if head_rows is not None:
            h = np.asarray(head_rows, F64)
            sel = (e >= head_off) & (e < head_off + h.shape[1])
            total[sel] += h[:, e[sel] - head_off].sum(axis=0)
        d = np.asarray(d, F64).copy()
        d[:n] += total
        segs.append(d)
        if clear_small:
            small_after[e] = 0.0
    out.update(seg_dst=segs, small=small_after, rows=rows_after,
               head_rows=None if head_rows is None else np.asarray(head_rows, F64).copy())
    return out
