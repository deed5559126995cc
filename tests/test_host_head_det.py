"""Deterministic mode for voxel-input fused FireNets and norm_input, what can be checked without a GPU: the float64 references of
tests/head_det_ref.py against torch.autograd and the reference's own lines, the geometry mirrors, that the bounds can fail, and
the ctypes table."""

import ctypes

import numpy as np
import pytest
import torch

import head_det_ref as HD
from event_flow_amd import _lib

F32, F64 = np.float32, np.float64


# ================================================================================================================ head wgrad
@pytest.mark.parametrize("case", HD.HEAD_CASES)
def test_head_wgrad_reference_is_autograds_conv2d_weight_gradient(case):
    x, g = HD.head_inputs(case, "real")
    ref, scale = HD.head_wgrad_ref64(x, g)
    xt = torch.from_numpy(x.astype(F64))
    w = torch.zeros(HD.C, case[1], 3, 3, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xt, w, padding=1)  # [B,32,H,W]
    y.backward(torch.from_numpy(g.astype(F64)).permute(0, 3, 1, 2))
    assert np.abs(w.grad.numpy() - ref).max() <= 1e-12 * max(scale.max(), 1.0)
    assert (scale >= np.abs(ref) * (1 - 1e-12)).all()


def test_head_wgrad_exact_leg_is_exact_in_float32():
    """The exact leg's claim: every product and partial sum is an integer multiple of 2^-6 below 2^18, whatever the order."""
    for case in HD.HEAD_CASES:
        for rep in (0, 1):
            x, g = HD.head_inputs(case, "exact", rep)
            ref, scale = HD.head_wgrad_ref64(x, g)
            assert np.array_equal(ref * 64, np.round(ref * 64)) and 2 * scale.max() * 64 < 2 ** 24
            assert np.array_equal(ref.astype(F32).astype(F64), ref)


def test_head_bound_rejects_a_dropped_border_tap_and_a_dropped_tail_channel():
    """The bar can fail: one term of a border pixel's tap left out, and the last output channel's terms of the last pixel."""
    for case in HD.HEAD_CASES:
        B, Cin, H, W = case
        x, g = HD.head_inputs(case, "real")
        x[B - 1, :, H - 1, W - 1] = 1.5  # (the pixel the mutants touch is not one of the empty ones)
        x[0, :, 0, 0] = -1.25
        ref, scale = HD.head_wgrad_ref64(x, g)
        assert HD.units(ref.astype(F32), ref, scale) <= 1.0 < HD.head_bound(*case)  # (the reference rounded once passes)
        tap = HD.head_wgrad_ref64(x, g, drop_tap=(0, 0, 0, Cin - 1, 1, 1))[0]  # pixel (0, 0), centre tap: a border pixel's term
        assert HD.units(tap, ref, scale) > HD.head_bound(*case, calls=2), case
        tail = HD.head_wgrad_ref64(x, g, drop_channel=HD.C - 1)[0]
        assert HD.units(tail, ref, scale) > HD.head_bound(*case, calls=2), case
        assert np.array_equal(tail[:HD.C - 1], ref[:HD.C - 1])


# ================================================================================================================ lif backward
class _Spike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, width):
        ctx.save_for_backward(x)
        ctx.kind, ctx.width = kind, width
        return (x > 0).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        sg = 1.0 / (1.0 + ctx.width * x * x) if ctx.kind == HD.ARCTAN else 1.0 / (1.0 + ctx.width * x.abs()) ** 2
        return g * sg, None, None


@pytest.mark.parametrize("hard", (True, False))
@pytest.mark.parametrize("surrogate", (HD.ARCTAN, HD.SUPERSPIKE))
@pytest.mark.parametrize("first", (False, True))
def test_lif_backward_sums_are_autograd_through_a_float64_cell(hard, surrogate, first):
    """The cell of spiking_submodules.py:103-126 restated in float64 -- v' = v lam (1 - z) + (1 - lam) cur (hard) or
    v lam + (1 - lam) cur - z th (soft), z' = spike(v' - th), lam = sigmoid(leak), th = clamp_min(thresh, 0.01), z detached -- with
    L = sum g_z z' + sum g_v v'.  The reference gets the cell's v' and must return autograd's gradients."""
    case = HD.LIF_CASES[1]
    d = HD.lif_inputs(case, first=first)
    npix = d["v_out"].shape[0]
    T = lambda a, grad=False: torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)  # noqa: E731
    cur = T(d["v_out"], True)  # (any float64 current will do; the potential follows from it)
    vp = T(np.zeros((npix, HD.C)) if d["v_prev"] is None else d["v_prev"], True)
    z = T(HD.unpack_bits(d["z_prev"], npix))
    leak, thresh = T(d["leak"], True), T(d["thresh"], True)
    lam, th = torch.sigmoid(leak), torch.clamp_min(thresh, 0.01)
    v = vp * lam * (1 - z) + (1 - lam) * cur if hard else vp * lam + (1 - lam) * cur - z * th
    zo = _Spike.apply(v - th, surrogate, HD.WIDTH[surrogate])
    L = (T(d["g_z"]) * zo).sum()
    if d["g_v"] is not None:
        L = L + (T(d["g_v"]) * v).sum()
    L.backward()
    for nblk in (1, HD.lif_bwd_grid(*case)):
        r = HD.lif_bwd_ref64(d, hard, surrogate, nblk, v_out64=v.detach().numpy())
        tol = 1e-10
        assert np.abs(r["g_cur"] - cur.grad.numpy()).max() < tol and np.abs(r["g_v_prev"] - vp.grad.numpy()).max() < tol
        assert np.abs(r["g_leak"] - leak.grad.numpy()).max() < tol * max(r["scale_leak"].max(), 1.0)
        assert np.abs(r["g_thresh"] - thresh.grad.numpy()).max() < tol * max(r["scale_thresh"].max(), 1.0)
        assert r["g_thresh"][HD.THRESH_FLOOR_CHANNEL] == 0.0 == float(thresh.grad[HD.THRESH_FLOOR_CHANNEL])
        assert (r["scale_leak"] >= np.abs(r["g_leak"]) * (1 - 1e-9)).all() and (r["scale_thresh"] >= np.abs(r["g_thresh"]) * (1 - 1e-9)).all()
        assert r["rows_leak"].shape == (nblk, HD.C)


def test_lif_bound_rejects_a_dropped_block():
    case = HD.LIF_CASES[1]
    d = HD.lif_inputs(case)
    nblk = HD.lif_bwd_grid(*case)
    r = HD.lif_bwd_ref64(d, True, HD.ARCTAN, nblk)
    assert HD.units(r["g_leak"].astype(F32), r["g_leak"], r["scale_leak"]) <= 1.0
    lost = r["rows_leak"][:-1].sum(0)  # the last block's row never added
    assert HD.units(lost, r["g_leak"], r["scale_leak"]) > HD.lif_bound(case, "leak")
    lost = r["rows_thresh"][:-1].sum(0)
    assert HD.units(lost, r["g_thresh"], r["scale_thresh"]) > HD.lif_bound(case, "thresh")


def test_lif_exact_leg_is_exact_in_float32_and_sees_one_lost_pixel():
    """The exact leg's claim: every block row and every total of g_leak / g_thresh is a float32 number whatever the order of the
    additions (multiples of 2^-7 far below 2^24 of them), and leaving out ONE pixel's term changes the total."""
    for case in HD.LIF_CASES:
        for hard in (True, False):
            d = HD.lif_exact_inputs(case)
            r = HD.lif_bwd_ref64(d, hard, HD.ARCTAN, HD.lif_bwd_grid(*case))
            for nm in ("rows_leak", "rows_thresh", "g_leak", "g_thresh", "scale_leak", "scale_thresh"):
                assert np.array_equal(r[nm] * 128, np.round(r[nm] * 128)), (case, hard, nm)
                assert np.abs(r[nm]).max() * 128 < 2 ** 24
            assert np.all(r["g_leak"] != 0) and r["g_thresh"][HD.THRESH_FLOOR_CHANNEL] == 0
            d2 = {k: (v.copy() if v is not None else None) for k, v in d.items()}
            d2["g_z"][0, 3] += 0.125  # one pixel, one channel
            r2 = HD.lif_bwd_ref64(d2, hard, HD.ARCTAN, HD.lif_bwd_grid(*case))
            assert r2["g_thresh"][3] != r["g_thresh"][3] and r2["g_leak"][3] != r["g_leak"][3]


# ================================================================================================================ norm_input
@pytest.mark.filterwarnings("ignore:std")  # (fewer than two non-zero entries: torch says so, and returns the NaN the test expects)
@pytest.mark.parametrize("n", HD.NORM_N[:-1] + (5000,))
@pytest.mark.parametrize("kind", ("voxel", "zeros", "one"))
def test_norm_reference_is_the_references_three_lines(n, kind):
    x = HD.norm_inputs(n, kind)
    ref, scale = HD.norm_ref64(x)
    t = torch.from_numpy(x.astype(F64)).clone()
    with np.errstate(all="ignore"):
        mean, stddev = t[t != 0].mean(), t[t != 0].std()  # models/model.py:247-252
        t[t != 0] = (t[t != 0] - mean) / stddev
    got = t.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max(initial=0.0) <= 1e-12 * max(scale.max(), 1.0)
    assert not np.signbit(ref[x == 0]).any() and (ref[x == 0] == 0).all()
    if kind == "one":
        assert np.isnan(ref).sum() == 1 and (x != 0).sum() == 1
    if kind == "voxel" and n >= 255:
        assert 0.6 < (x == 0).mean() < 0.8 and np.signbit(x[x == 0]).any()


def test_norm_bound_rejects_a_biased_std():
    x = HD.norm_inputs(1025, "voxel")
    ref, scale = HD.norm_ref64(x)
    assert HD.units(ref.astype(F32), ref, scale) <= 1.0 < HD.NORM_OPS
    k = int((x != 0).sum())
    assert HD.units(ref * np.sqrt(k / (k - 1.0)), ref, scale) > HD.NORM_OPS  # (std with 1 / k)


# ================================================================================================================ geometry
def test_geometry_mirrors_are_monotone_and_capped():
    prev = 0
    for bh in range(1, 1500):
        n = HD.head_wgrad_det_slabs(1, bh, 7)
        assert prev <= n <= HD.HEAD_BLOCK_CAP == 256 and n * 4 >= min(bh, 1024) and n == HD.head_wgrad_det_slabs(bh, 1, 99)
        prev = n
    assert prev == 256 and HD.head_wgrad_det_slabs(5, 208, 8) == 256 and HD.head_wgrad_det_slabs(1, 3, 5) == 1
    prev = 0
    for npix in list(range(1, 200)) + list(range(200, 40000, 97)):
        n = HD.lif_bwd_grid(1, 1, npix)
        assert prev <= n <= HD.LIF_BLOCK_CAP == 768 and n * 256 >= min(npix * 8, 768 * 256)
        assert HD.lif_bwd_grid(1, 1, npix, 3) == min(n, 3)
        prev = n
    assert prev == 768 and HD.lif_bwd_grid(1, 160, 160) == 768 and HD.lif_bwd_grid(1, 160, 160, 512) == 512
    prev = 0
    for n_ in list(range(1, 5000, 13)) + [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 5, 2 ** 24]:
        n = HD.norm_grid(n_)
        assert prev <= n <= HD.NORM_BLOCK_CAP == 1024 and n * 1024 >= min(n_, 2 ** 20) and HD.norm_ws(n_) == 3 * n
        prev = n
    assert prev == 1024 and HD.norm_grid(1024) == 1 and HD.norm_grid(1025) == 2


def test_the_library_states_the_same_geometry():
    """The two host-side size functions against their mirrors (no GPU: nothing is launched); zero for what the calls refuse."""
    from event_flow_amd import build
    build.build(verbose=False)
    L = _lib.load()
    for B, H, W in [(1, 3, 5), (2, 5, 8), (5, 208, 8), (1, 1, 1), (8, 128, 128), (3, 341, 2), (1, 1023, 4), (1, 1025, 4)]:
        assert L.evf_head_wgrad_det_slabs(B, H, W) == HD.head_wgrad_det_slabs(B, H, W)
    assert L.evf_head_wgrad_det_slabs(0, 4, 4) == 0 == L.evf_head_wgrad_det_slabs(2, 0, 4)
    for n in HD.NORM_N + (2 ** 20, 2 ** 20 + 1, 2 ** 31 + 7):
        assert L.evf_norm_nonzero_det_ws(n) == HD.norm_ws(n)
    assert L.evf_norm_nonzero_det_ws(0) == 0 == L.evf_norm_nonzero_det_ws(-3)


def test_chains_count_the_longest_path():
    assert HD.head_chain(1, 1, 3, 5) == 8 + 2 + 17           # one row per wave, one step of eight; the tree; one slab row
    assert HD.head_chain(5, 5, 208, 8) == 16 + 2 + 32        # two trips
    assert HD.head_chain(5, 5, 208, 8, calls=2) == 32 + 4 + 1 + 32
    assert HD.lif_chain(1, 160, 160, 512) == 2 + 8 + 48      # two trips on 512 blocks
    assert HD.lif_chain(2, 32, 40, 3) == 27 + 8 + 17


# ================================================================================================================ C ABI table
def test_the_ctypes_table_knows_the_five_entry_points():
    S, P, I, F, L = _lib.SIGNATURES, _lib.P, _lib.I, _lib.F, _lib.L
    assert S["evf_head_wgrad_det_slabs"] == [I, I, I]
    assert S["evf_head_wgrad_det"] == S["evf_head_wgrad"][:-1] + [I, P]
    assert S["evf_lif_bwd_det"] == S["evf_lif_bwd"][:-1] + [I, I, P]
    assert S["evf_norm_nonzero_det_ws"] == [L]
    assert S["evf_norm_nonzero_det"] == [P, L, P, P, L, P]
    assert _lib.RESTYPES["evf_norm_nonzero_det_ws"] is ctypes.c_int64
    assert "evf_head_wgrad_det_slabs" not in _lib.RESTYPES
