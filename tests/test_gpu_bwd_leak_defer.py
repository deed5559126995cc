"""The leak gradient of a hidden LIF cell without its v_prev stream (include/evflow.h, evf_bwd_leak_defer): a window of three
passes of one cell through evf_lif_bwd_wgrad2, every pass forming its whole leak term (bits off) against every pass but the
first leaving the half that needs v_prev to the pass before (16 | 32, the first pass 32).  B = 2, H = 6, W = 70 (a clamped tail
unit, three blocks), potentials straddling the threshold, a feed-forward and a recurrent cell, a state entering the window and
a NULL one, cells launched one by one and recorded (k_bwd_diag_ws<8>).  The PLIF-family entry points ignore the bits (their
kernels have no registers to spare) and are not exercised here."""

import os
import subprocess
import sys

import pytest
import torch

from event_flow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 32
B, H, W, T = 2, 6, 70, 3
ROW_LD = 160
WIDTH = 10.0
BAR = 2e-5  # the bar of the cell tests for per-channel sums (tests/test_gpu_kernels.py)
SKIP, COLLECT = 16, 32
P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731


def _words(z):  # [B,H,W,32] bool -> [B,H,W] int32 spike words (bit c = channel c)
    w = torch.zeros(z.shape[:3], dtype=torch.int64, device=z.device)
    for c in range(32):
        w |= z[..., c].long() << c
    return torch.where(w < 2**31, w, w - 2**32).to(torch.int32).contiguous()


def _planes(bits):
    t = torch.empty(B, H, 32, (W + 31) // 32, dtype=torch.int32, device=DEV)
    _lib.call("evf_bits_transpose", P(bits), B, H, W, P(t))
    return t


def _chain(rec, null_state, small_channel=None, seed=5):
    torch.manual_seed(seed)
    f = lambda *s, scale=1.0: torch.randn(*s, device=DEV) * scale  # noqa: E731
    ch = {"rec": rec, "leak": f(32, scale=0.3), "thresh": f(32, scale=0.1) + 0.4}
    if small_channel is not None:
        ch["leak"][small_channel] = -12.0  # lam = 6.1e-6, below the kernel's threshold (raw parameter < -11)
    th = ch["thresh"].clamp_min(0.01)
    ch["v"] = [f(B, H, W, C, scale=0.6) + 0.3 for _ in range(T + 1)]  # v[t]: before pass t, v[t + 1]: after it
    ch["zb"] = [_words(v > th) for v in ch["v"][:T]]  # spikes before pass t: both values
    if null_state:
        ch["v"][0], ch["zb"][0] = None, None
    ch["xT"] = [_planes(_words(torch.rand(B, H, W, 32, device=DEV) < 0.15)) for _ in range(T)]
    ch["zT"] = [_planes(z) if (rec and z is not None) else None for z in ch["zb"]]
    ch["gz"] = [f(B, H, W, C, scale=0.2) for _ in range(T)]
    ch["gz2"] = [f(B, H, W, C, scale=0.2) if rec else None for _ in range(T)]
    return ch


def _run(ch, flags, recorded=False):
    """The window's passes last to first; flags(t) -> the FB_LD bits of pass t.  -> per-pass outputs."""
    L = _lib.load()
    nsl = L.evf_lif_bwd_wgrad_slabs(B, H, W)
    gv = torch.full((B, H, W, C), 3.0, device=DEV)  # dL/dv carried in place, like the engine's
    sff, srec = torch.full((nsl, 9216), 5.0, device=DEV), torch.full((nsl, 9216), 5.0, device=DEV)
    out = {"gcur": [], "gsp": [], "gvp": [], "rows": [], "sff": sff, "srec": srec}
    acc_ff = acc_rec = 0
    for t in range(T - 1, -1, -1):
        gcur = torch.full((B, H, W, C), 3.0, device=DEV)
        gsp = torch.zeros(3, B, H, W, C, dtype=torch.bfloat16, device=DEV)
        rows = torch.zeros(nsl, ROW_LD, device=DEV)
        use_rec = ch["rec"] and ch["zb"][t] is not None
        if use_rec and not acc_rec and acc_ff:
            srec.zero_()
        if recorded:
            assert _lib.raw("evf_bwd_defer_begin") == 0 and _lib.raw("evf_bwd_defer_slot", 2) == 0
        try:
            _lib.call("evf_lif_bwd_wgrad2", P(ch["gz"][t]), P(ch["gz2"][t]), P(gv) if t < T - 1 else None, P(ch["v"][t + 1]), P(ch["v"][t]),
                      P(ch["zb"][t]), P(ch["xT"][t]), P(ch["zT"][t]) if use_rec else None, P(ch["leak"]), P(ch["thresh"]), B, H, W, 1, 0, WIDTH,
                      P(gcur), P(gsp), P(gv), P(rows[:, :32]), P(rows[:, 32:]), P(sff), P(srec) if use_rec else None,
                      acc_ff | flags(t) | (ROW_LD << 8))
        finally:
            if recorded:
                _lib.call("evf_bwd_defer_flush")
        acc_ff = 1
        acc_rec = acc_rec or use_rec
        out["gcur"].append(gcur), out["gsp"].append(gsp), out["gvp"].append(gv.clone()), out["rows"].append(rows.sum(0))
    torch.cuda.synchronize()
    out["g_leak"] = torch.stack([r[:32] for r in out["rows"]]).sum(0)
    out["g_thresh"] = torch.stack([r[32:64] for r in out["rows"]]).sum(0)
    return out


def _reference(ch):
    """float64 on the CPU: per pass (last first) the per-channel sums of gv * (vp * (1 - z) - cur) * sigmoid'(leak), the part of
    each that needs only v_out, and the largest single term."""
    d = lambda x: x.double().cpu()  # noqa: E731
    lam = torch.sigmoid(d(ch["leak"]))
    th = d(ch["thresh"]).clamp_min(0.01)
    gv_in = torch.zeros(B, H, W, C, dtype=torch.float64)
    full, vo_half, largest = [], [], 0.0
    for t in range(T - 1, -1, -1):
        vo = d(ch["v"][t + 1])
        vp = d(ch["v"][t]) if ch["v"][t] is not None else torch.zeros_like(vo)
        if ch["zb"][t] is not None:
            zw = ch["zb"][t].cpu().long()
            z = torch.stack([(zw >> c) & 1 for c in range(32)], -1).double()
        else:
            z = torch.zeros_like(vo)
        sg = 1.0 / (1.0 + WIDTH * (vo - th) ** 2)
        gz = d(ch["gz"][t]) + (d(ch["gz2"][t]) if ch["gz2"][t] is not None else 0.0)
        gv = gv_in + gz * sg
        cur = (vo - vp * lam * (1 - z)) / (1 - lam)
        term = gv * (vp * (1 - z) - cur) * lam * (1 - lam)
        full.append(term.sum((0, 1, 2)))
        vo_half.append((-gv * vo / (1 - lam) * lam * (1 - lam)).sum((0, 1, 2)))
        largest = max(largest, float(term.abs().max()))
        gv_in = gv * lam * (1 - z)
    return full, vo_half, largest


def _dist(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


OFF = lambda t: 0  # noqa: E731
ON = lambda t: (SKIP | COLLECT) if t > 0 else COLLECT  # noqa: E731


@pytest.mark.parametrize("recorded", [False, True])
@pytest.mark.parametrize("null_state", [False, True])
@pytest.mark.parametrize("rec", [False, True])
def test_deferred_leak_gradient_matches_the_whole_form(rec, null_state, recorded):
    """g_cur, its split planes, g_v_prev, g_thresh and the slabs bit for bit between the two forms; g_leak over the window against
    the float64 sum: the old form below the cell tests' bar, the new form within 2 x the old form's distance + one fp32 ulp of
    the largest term (both are fp32 sums of as many terms, grouped by another pass).
    Measured on an MI355X (old / new distance, relative to the largest |reference| channel; one ulp of the largest term 1.4e-8 ...
    1.9e-8): feed-forward 2.31e-7 / 1.63e-7 (NULL entering state 2.01e-7 / 0.94e-7), recurrent 2.01e-7 / 1.35e-7 (NULL 1.50e-7 /
    1.34e-7); the same figures recorded and launched one by one."""
    assert _lib.load().evf_bwd_leak_defer() == 1
    ch = _chain(rec, null_state)
    old, new = _run(ch, OFF, recorded), _run(ch, ON, recorded)
    for k in ("gcur", "gsp", "gvp"):
        for t in range(T):
            assert torch.equal(old[k][t], new[k][t]), (k, t)
    assert torch.equal(old["g_thresh"], new["g_thresh"])
    assert torch.equal(old["sff"], new["sff"]) and torch.equal(old["srec"], new["srec"])
    full, _, largest = _reference(ch)
    ref = torch.stack(full).sum(0)
    d_old, d_new = _dist(old["g_leak"], ref), _dist(new["g_leak"], ref)
    ulp = largest * 2.0**-23 / float(ref.abs().max())
    print(f"leak defer rec={rec} null={null_state} recorded={recorded}: old {d_old:.3e} new {d_new:.3e} ulp(largest term) {ulp:.3e}")
    assert float(ref.abs().max()) > 0 and d_old < BAR
    assert d_new <= 2 * d_old + ulp
    assert not torch.equal(old["g_leak"], new["g_leak"])  # (the new form did run)


@pytest.mark.parametrize("rec", [False, True])
def test_last_pass_adds_only_its_own_half(rec):
    """The window's last pass has no carried dL/dv: with both bits on, its g_leak is the sum of -gv * vo / (1 - lam) alone."""
    ch = _chain(rec, False)
    new = _run(ch, ON)
    _, vo_half, _ = _reference(ch)
    d = _dist(new["rows"][0][:32], vo_half[0])
    print(f"last pass rec={rec}: {d:.3e}")
    assert d < BAR


def test_small_lam_channels_keep_the_old_form():
    """A channel whose lam is below the kernel's threshold: its quad loads v_prev and forms the old terms on every pass -- the
    same bits as with the switch off; the other quads use the new form and stay within the bound of the first test."""
    c0 = 9
    ch = _chain(True, False, small_channel=c0)
    old, new = _run(ch, OFF), _run(ch, ON)
    quad = slice(4 * (c0 // 4), 4 * (c0 // 4) + 4)
    full, _, largest = _reference(ch)
    ref = torch.stack(full).sum(0)
    dq = float((new["g_leak"][c0].double().cpu() - ref[c0]).abs() / ref[c0].abs())
    print(f"small lam: channel {c0} new {float(new['g_leak'][c0]):.6e} old {float(old['g_leak'][c0]):.6e} ref {float(ref[c0]):.6e} rel {dq:.3e}")
    assert float(ref[c0].abs()) > 0 and dq < BAR
    assert torch.equal(new["g_leak"][quad], old["g_leak"][quad])
    others = torch.ones(32, dtype=torch.bool)
    others[quad] = False
    d_old = float((old["g_leak"].double().cpu() - ref)[others].abs().max() / ref[others].abs().max())
    d_new = float((new["g_leak"].double().cpu() - ref)[others].abs().max() / ref[others].abs().max())
    ulp = largest * 2.0**-23 / float(ref[others].abs().max())
    print(f"small lam: other channels old {d_old:.3e} new {d_new:.3e}")
    assert d_old < BAR and d_new <= 2 * d_old + ulp
    assert not torch.equal(new["g_leak"][others.to(DEV)], old["g_leak"][others.to(DEV)])


def test_environment_switch_restores_the_old_form(tmp_path):
    """EVF_BWD_LEAK_DEFER=0 (read when the library first needs it: a fresh process): the bits are ignored, g_leak is the old
    form's bit for bit."""
    ch = _chain(True, False)
    old = _run(ch, OFF)
    dst = tmp_path / "g_leak.pt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVF_BWD_LEAK_DEFER="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.abspath(__file__), str(dst)], check=True, env=env, cwd=root, timeout=300)
    got = torch.load(dst)
    assert got["honoured"] == 0
    assert torch.equal(got["g_leak"], old["g_leak"].cpu())
    for t in range(T):
        assert torch.equal(got["gvp"][t], old["gvp"][t].cpu())


if __name__ == "__main__":  # the child of test_environment_switch_restores_the_old_form
    ch_ = _chain(True, False)
    o_ = _run(ch_, ON)
    torch.save({"honoured": _lib.load().evf_bwd_leak_defer(), "g_leak": o_["g_leak"].cpu(), "gvp": [g.cpu() for g in o_["gvp"]]}, sys.argv[1])
