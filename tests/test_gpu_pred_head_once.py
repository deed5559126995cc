"""The prediction head inside the top hidden layer, evaluated once per pixel: team E of the forward kernels splits the head's
two components over the eight lanes of a pixel (k_fwd_win_t / k_fwd_diag_t), team E of the backward kernels loads the head's
operands once per pixel and hands tanh' round by DPP moves (k_bwd_win_lif_top and the one-pass form).  Checked on the smallest
shapes at which these paths can go wrong -- one full 64-pixel unit plus a 6-pixel partial one with partial 32-pixel strips, and
the minimal full tile --, windows of three passes and of one, the first pass from the NULL state, a third of the units spiking
(all-zero spike words would hide a wrong lane exchange)."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from event_flow_amd import _lib
from test_gpu_kernels import C, DEV, P, _bits, _f, _packs, _planes, _rel

pytestmark = pytest.mark.gpu

SHAPES = [(2, 6, 70), (1, 2, 32)]
NPASS = [3, 1]
WIDTH = 10.0


def _unpack(words):
    """int32 spike words [...] -> float64 [..., 32]"""
    w = words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return ((w[..., None] >> np.arange(32)) & 1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _forward(shape, npass):
    """The top layer's passes through the window launch (one chain under one index; a window of one pass is a diagonal launch of
    one cell) and through one diagonal launch per pass.  Computed once, shared, never modified."""
    B, H, W = shape
    torch.manual_seed(53)
    L = _lib.load()
    nW = (W + 31) // 32
    xs = [_bits(B, H, W, 0.3) for _ in range(npass)]
    wff = _packs()[0]
    leak = _f(32, scale=0.1) - 1
    pw, pb = _f(2, 32, scale=0.2), _f(2, scale=0.1)
    # thresholds: per channel the 2/3 quantile of the first pass's potential -> a third of the units spike
    v1, z1 = torch.empty(B, H, W, C, device=DEV), torch.empty(B, H, W, dtype=torch.int32, device=DEV)
    zT1 = torch.empty(B, H, 32, nW, dtype=torch.int32, device=DEV)
    _lib.call("evf_conv_lif_fwd_b3", P(xs[0]), P(wff), None, P(leak), P(torch.full((32,), 1e9, device=DEV)), None, None, B, H, W, 1, P(v1),
              P(z1), P(zT1))
    thresh = torch.quantile(v1.reshape(-1, C), 2.0 / 3.0, dim=0).clamp_min(0.02).contiguous()

    def outs():
        return [dict(v=torch.full((B, H, W, C), 7.0, device=DEV), z=torch.full((B, H, W), 5, dtype=torch.int32, device=DEV),
                     zT=torch.full((B, H, 32, nW), 5, dtype=torch.int32, device=DEV), flow=torch.full((B, 2, H, W), 7.0, device=DEV))
                for _ in range(npass)]

    def cell(o, t):
        _lib.call("evf_conv_lif_fwd_b3_pred", P(xs[t]), P(wff), None, P(leak), P(thresh), P(o[t - 1]["v"]) if t else None,
                  P(o[t - 1]["z"]) if t else None, B, H, W, 1, P(o[t]["v"]), P(o[t]["z"]), P(o[t]["zT"]), P(pw), P(pb), P(o[t]["flow"]))

    res = {}
    assert L.evf_fwd_diag_select(2) == 0
    try:
        for mode in ("win", "diag"):
            o = outs()
            for grp in ([list(range(npass))] if mode == "win" else [[t] for t in range(npass)]):
                assert _lib.raw("evf_fwd_defer_begin") == 0
                try:
                    for t in grp:
                        assert _lib.raw("evf_fwd_defer_slot", 0) == 0
                        cell(o, t)
                    assert _lib.raw("evf_fwd_defer_pending") == len(grp)
                finally:
                    _lib.call("evf_fwd_defer_flush")
            torch.cuda.synchronize()
            res[mode] = o
    finally:
        L.evf_fwd_diag_select(-1)
    return dict(xs=xs, leak=leak, thresh=thresh, pw=pw, pb=pb, **res)


@pytest.mark.parametrize("npass", NPASS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["win", "diag"])
def test_fused_head_forward_is_evf_pred_fwd_of_the_spikes_it_wrote(shape, npass, mode):
    """flow of the fused top layer == evf_pred_fwd (untouched: an independent reference) of the spike words the same launch wrote,
    bit for bit; against float64: |d| <= (33 sum_c |w_c| + 4) 2^-24 per component (the in-order fp32 sum of 32 terms plus the bias,
    and tanhf)."""
    B, H, W = shape
    F = _forward(shape, npass)
    pw64, pb64 = F["pw"].double().cpu().numpy(), F["pb"].double().cpu().numpy()
    bound = (33.0 * np.abs(pw64).sum(axis=1) + 4.0) * 2.0**-24  # [2]
    rate = []
    for t in range(npass):
        o = F[mode][t]
        ref = torch.empty(B, 2, H, W, device=DEV)
        _lib.call("evf_pred_fwd", P(o["z"]), P(F["pw"]), P(F["pb"]), B, H, W, P(ref))
        torch.cuda.synchronize()
        assert torch.equal(o["flow"], ref), (t, int((o["flow"] != ref).sum()))
        z = _unpack(o["z"])  # [B,H,W,32]
        rate.append(z.mean())
        f64 = np.tanh(np.einsum("bhwc,oc->bohw", z, pw64) + pb64[None, :, None, None])
        err = np.abs(o["flow"].double().cpu().numpy() - f64).max(axis=(0, 2, 3))
        print(f"pass {t}: spike rate {z.mean():.3f}, |flow - fp64| max {err} bound {bound}")
        assert (err <= bound).all(), (t, err, bound)
        assert torch.equal(o["v"], F["win"][t]["v"]) and torch.equal(o["z"], F["win"][t]["z"]) and torch.equal(o["zT"], F["win"][t]["zT"])
    assert 0.2 < rate[0] < 0.45, rate  # (a third of the units spike at the first pass)


def _cell_backward_fp64(F, o, gfl, npass):
    """dL/d(current) of every pass in float64: autograd of spiking_submodules.py:103-126 (hard reset, arctan surrogate, previous
    spikes detached) under the head (tanh of a 1x1 conv of the spikes), written out."""
    lam = 1.0 / (1.0 + np.exp(-F["leak"].double().cpu().numpy()))
    th = np.maximum(F["thresh"].double().cpu().numpy(), 0.01)
    pw = F["pw"].double().cpu().numpy()
    gv, out = 0.0, [None] * npass
    for t in range(npass - 1, -1, -1):
        flow, g = o[t]["flow"].double().cpu().numpy(), gfl[t].double().cpu().numpy()
        gpre = g * (1.0 - flow * flow)                            # [B,2,H,W]
        gz = np.einsum("bohw,oc->bhwc", gpre, pw)                 # dL/d(spikes)
        x = o[t]["v"].double().cpu().numpy() - th
        gvt = gv + gz / (1.0 + WIDTH * x * x)                     # dL/dv' of the pass
        out[t] = gvt * (1.0 - lam)
        zprev = _unpack(o[t - 1]["z"]) if t else 0.0
        gv = gvt * lam * (1.0 - zprev)
    return out, gv


@functools.lru_cache(maxsize=None)
def _backward(shape, npass):
    """The top layer's backward on the tape of _forward: one evf_lif_bwd_wgrad_top launch per pass (`ref`) and the window launch with
    the head inside (`got`).  Computed once, shared, never modified."""
    B, H, W = shape
    F = _forward(shape, npass)
    o = F["win"]
    torch.manual_seed(59)
    L = _lib.load()
    nsl = max(L.evf_lif_bwd_wgrad_slabs(B, H, W), 512)
    row_ld = 224
    leak, thresh, pw = F["leak"], F["thresh"], F["pw"]
    vs = [None] + [o[t]["v"] for t in range(npass)]
    zs = [None] + [o[t]["z"] for t in range(npass - 1)]
    xT = [_planes(x) for x in F["xs"]]
    flows, zo = [o[t]["flow"] for t in range(npass)], [o[t]["z"] for t in range(npass)]
    gfl = [_f(B, 2, H, W) for _ in range(npass)]
    arr = lambda ts: (ctypes.c_void_p * npass)(*[P(x) for x in ts])  # noqa: E731
    order = list(range(npass - 1, -1, -1))

    def outs():
        return {"gcur": [torch.full((B, H, W, C), 3.0, device=DEV) for _ in range(npass)],
                "gsp": [torch.zeros(3, B, H, W, C, dtype=torch.bfloat16, device=DEV) for _ in range(npass)],
                "gv": torch.full((B, H, W, C), 3.0, device=DEV), "rows": torch.zeros(nsl, row_ld, device=DEV),
                "slab": torch.full((nsl, 9216), 5.0, device=DEV)}

    ref, got = outs(), outs()
    for k in range(npass):
        t = npass - 1 - k
        flag = (1 if k else 0) | (row_ld << 8)
        _lib.call("evf_lif_bwd_wgrad_top", P(flows[t]), P(gfl[t]), P(pw), P(zo[t]), P(ref["rows"][:, 128:]), P(ref["rows"][:, 192:]),
                  P(ref["gv"]) if k else None, P(vs[t + 1]), P(vs[t]), P(zs[t]), P(xT[t]), P(leak), P(thresh), B, H, W, 1, 0, WIDTH,
                  P(ref["gcur"][t]), P(ref["gsp"][t]), P(ref["gv"]), P(ref["rows"][:, :32]), P(ref["rows"][:, 32:]), P(ref["slab"]), flag)
    _lib.call("evf_lif_bwd_wgrad_window", npass, None, arr([flows[t] for t in order]), arr([gfl[t] for t in order]), P(pw),
              arr([zo[t] for t in order]), P(got["rows"][:, 128:]), P(got["rows"][:, 192:]), arr([vs[t + 1] for t in order]),
              arr([vs[t] for t in order]), arr([zs[t] for t in order]), arr([xT[t] for t in order]), arr([got["gcur"][t] for t in order]),
              arr([got["gsp"][t] for t in order]), P(leak), P(thresh), B, H, W, WIDTH, P(got["gv"]), P(got["rows"][:, :32]),
              P(got["rows"][:, 32:]), P(got["slab"]), 0 | (row_ld << 8))
    torch.cuda.synchronize()
    return ref, got, gfl


@pytest.mark.parametrize("npass", NPASS)
@pytest.mark.parametrize("shape", SHAPES)
def test_top_layer_window_backward_with_the_head_once_per_pixel(shape, npass):
    """evf_lif_bwd_wgrad_window with the head inside against one evf_lif_bwd_wgrad_top launch per pass, on the tape the fused forward
    wrote: dL/d(current) (fp32, its three bf16 planes and their sum) and the carried dL/dv bit for bit, the pred.w / pred.b / leak /
    threshold rows and the slab to round-off (the bars of test_lif_hidden_cell_backward_of_a_window_in_one_launch); dL/d(current)
    and the carried dL/dv against float64 to 2e-6 of their norm (the bar of the top-layer window tests of test_gpu_network.py)."""
    F = _forward(shape, npass)
    o = F["win"]
    ref, got, gfl = _backward(shape, npass)
    g64, gv64 = _cell_backward_fp64(F, o, gfl, npass)
    for t in range(npass):
        assert torch.equal(ref["gcur"][t], got["gcur"][t]), ("g_cur", t)
        assert torch.equal(ref["gsp"][t], got["gsp"][t]), ("g_split", t)
        for which in (ref, got):
            rec = which["gsp"][t][0].float() + which["gsp"][t][1].float() + which["gsp"][t][2].float()
            assert torch.equal(rec, which["gcur"][t]), ("planes' sum", t)  # (the split is exact)
        a = got["gcur"][t].double().cpu().numpy()
        e = float(np.linalg.norm(a - g64[t]) / np.linalg.norm(g64[t]))
        print(f"pass {t}: |g_cur - fp64| / |fp64| = {e:.3e}")
        assert np.linalg.norm(g64[t]) > 0 and e < 2e-6, (t, e)
    assert torch.equal(ref["gv"], got["gv"]) and float(ref["gv"].abs().max()) > 0
    e = float(np.linalg.norm(got["gv"].double().cpu().numpy() - gv64) / np.linalg.norm(gv64))
    print(f"carried dL/dv: |got - fp64| / |fp64| = {e:.3e}")
    assert e < 2e-6, e
    for name in ("slab", "rows"):
        r = _rel(got[name].sum(0), ref[name].sum(0))
        print(f"{name}: window against per-pass launches {r:.3e}")
        assert r < 2e-5, (name, r)
    # the head's own rows, in float64: dWp[o][c] = sum gpre_o * z_c, db[o] = sum gpre_o
    dw64, db64 = np.zeros((2, 32)), np.zeros(2)
    for t in range(npass):
        flow, g = o[t]["flow"].double().cpu().numpy(), gfl[t].double().cpu().numpy()
        gpre = g * (1.0 - flow * flow)
        dw64 += np.einsum("bohw,bhwc->oc", gpre, _unpack(o[t]["z"]))
        db64 += gpre.sum(axis=(0, 2, 3))
    rows = got["rows"].sum(0).double().cpu().numpy()
    for name, a, b in (("pred.w", rows[128:192].reshape(2, 32), dw64), ("pred.b", rows[192:194], db64)):
        r = float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
        print(f"{name}: against fp64 {r:.3e}")
        assert r < 2e-5, (name, r)
