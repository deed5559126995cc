"""The head layer's backward of a window in the epilogue of its input-gradient products (k_dgrad_head_win,
csrc/evf_head_dgrad.hip) against the path it replaces: the products through evf_conv_dgrad_b3 into one dL/d(spikes) buffer per
pass, then evf_head_lif_bwd_wgrad over those buffers (k_head_bwd_win / k_head_bwd_mfma).  Both recorded, as the engine does.

  * dL/dv leaving the window: bit for bit (the product and the element-wise expression are the same);
  * the weight-gradient slab and the per-channel rows, summed over rows: other grouping of the same partial sums -- the largest
    error against a float64 reference on the CPU is at most twice the old path's on the same inputs;
  * the predicate, the switch, and one engine-level step with the switch on and off.

EVF_HEAD_DGRAD_REPORT=<file>: the two errors of every case are appended there (profiles/head_dgrad_win_report.txt)."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from event_flow_amd import _lib
from event_flow_amd.models.spiking_util import SURROGATE_ID

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 32
WIDTH = 10.0
ARCTAN = SURROGATE_ID["arctanspike"]
ENOTSUP = -95
P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731


def _inputs(B, Cin, H, W, npass, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = {"leak": R(C) * 0.3, "thresh": R(C) * 0.1 + 0.5, "wt": (torch.rand(C, C, 3, 3, generator=g) * 2 - 1) * 0.2,
         "xs": [torch.poisson(torch.full((B, Cin, H, W), 0.4), generator=g) for _ in range(npass)],
         "vs": [R(B, H, W, C) * 0.7 for _ in range(npass + 1)],  # vs[t]: potential before pass t, vs[t + 1]: behind it
         "zs": [torch.randint(-2 ** 31, 2 ** 31 - 1, (B, H, W), generator=g, dtype=torch.int64).to(torch.int32) for _ in range(npass)],
         "gv_in": R(B, H, W, C) * 0.1}
    planes = []  # backward pass k: the exact three-way bf16 split of a random dL/d(current) of the layer above
    for _ in range(npass):
        gc = R(B, H, W, C) * 0.2
        hi = gc.bfloat16()
        mid = (gc - hi.float()).bfloat16()
        lo = (gc - hi.float() - mid.float()).bfloat16()
        planes.append(torch.stack([hi, mid, lo]).contiguous())
    d["planes"] = planes
    return d


def _reference(d, B, Cin, H, W, npass, carry_in, width=WIDTH):
    """float64 on the CPU: the slab's row sum [32][Cin * 9], the leak / thresh sums [32], dL/dv leaving the window."""
    lam = torch.sigmoid(d["leak"].double())
    th = d["thresh"].double().clamp_min(0.01)
    gv = d["gv_in"].double() if carry_in else torch.zeros(B, H, W, C, dtype=torch.float64)
    dw = torch.zeros(C, Cin * 9, dtype=torch.float64)
    sl, st = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    shifts = torch.arange(C)
    for k in range(npass):
        t = npass - 1 - k
        g = d["planes"][k].double().sum(0)  # [B,H,W,32]
        gz = F.conv_transpose2d(g.permute(0, 3, 1, 2), d["wt"].double(), padding=1).permute(0, 2, 3, 1)
        vo = d["vs"][t + 1].double()
        vp = d["vs"][t].double() if t else torch.zeros_like(vo)
        z = ((d["zs"][t].to(torch.int64).unsqueeze(-1) >> shifts) & 1).double() if t else torch.zeros_like(vo)
        sg = 1.0 / (1.0 + width * (vo - th) ** 2)
        gsp = gz * sg
        gvt = gv + gsp
        gc = gvt * (1.0 - lam)
        cur = (vo - vp * lam * (1.0 - z)) / (1.0 - lam)
        dlam = vp * (1.0 - z) - cur
        sl += (gvt * dlam).sum((0, 1, 2))
        st -= gsp.sum((0, 1, 2))
        xu = F.unfold(d["xs"][t].double(), 3, padding=1)  # [B, Cin * 9, H * W]
        dw += torch.einsum("bkp,bpc->ck", xu, gc.reshape(B, H * W, C))
        gv = gvt * lam * (1.0 - z)
    g_leak = sl * lam * (1.0 - lam)
    g_thresh = torch.where(d["thresh"].double() > 0.01, st, torch.zeros_like(st))
    return dw, g_leak, g_thresh, gv


def _run(d, B, Cin, H, W, npass, fused, carry_in, acc0):
    L = _lib.load()
    nsl = L.evf_head_lif_bwd_wgrad_slabs(B, H, W)
    row_ld = 64
    dev = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in d.items()}
    pb3 = torch.empty(54 * 1024, dtype=torch.uint8, device=DEV)
    _lib.call("evf_pack_conv_weight_b3t", P(dev["wt"]), C, C, P(pb3))
    gv = dev["gv_in"].clone() if carry_in else torch.empty(B, H, W, C, device=DEV)
    slab = torch.full((nsl, C * Cin * 9), 0.5 if acc0 else 7.0, device=DEV)
    rows = torch.zeros(nsl, row_ld, device=DEV)
    gzs = [torch.empty(B, H, W, C, device=DEV) for _ in range(npass)]
    assert _lib.raw("evf_bwd_defer_begin") == 0
    try:
        for k in range(npass):  # backward pass k = forward pass npass - 1 - k
            t = npass - 1 - k
            tail = (P(gv) if (k or carry_in) else None, P(dev["vs"][t + 1]), P(dev["vs"][t]) if t else None, P(dev["zs"][t]) if t else None,
                    P(dev["xs"][t]), P(dev["leak"]), P(dev["thresh"]), B, Cin, H, W, 1, ARCTAN, WIDTH)
            out = (P(gv), P(rows[:, :32]), P(rows[:, 32:]), P(slab), (1 if (k or acc0) else 0) | (row_ld << 8))
            if fused:
                assert _lib.raw("evf_bwd_defer_slot", 2 * k + 1) == 0
                _lib.call("evf_head_bwd_dgrad_win", P(dev["planes"][k]), P(pb3), *tail, *out)
            else:
                assert _lib.raw("evf_bwd_defer_slot", 2 * k) == 0
                _lib.call("evf_conv_dgrad_b3", P(dev["planes"][k]), P(pb3), P(gzs[k]), 0, B, H, W, None, None)
                assert _lib.raw("evf_bwd_defer_slot", 2 * k + 1) == 0
                _lib.call("evf_head_lif_bwd_wgrad", P(gzs[k]), *tail, None, *out)
        assert _lib.raw("evf_bwd_defer_pending") == (npass if fused else 2 * npass)
    finally:
        _lib.call("evf_bwd_defer_flush")
    torch.cuda.synchronize()
    return gv.cpu(), slab.cpu().double().sum(0).view(C, Cin * 9), rows.cpu().double().sum(0)


def _err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.fixture(autouse=True)
def _default_switches():
    yield
    _lib.load().evf_head_dgrad_win_select(-1, 0)


# (B, H, W, Cin, passes, grid override, dL/dv carried into the window, slab accumulated from the first pass on)
CASES = [(1, 4, 32, 2, 1, 0, False, False), (1, 4, 32, 2, 2, 0, True, False), (1, 4, 32, 2, 4, 0, False, True),
         (2, 8, 64, 2, 1, 0, True, True), (2, 8, 64, 2, 2, 0, False, False), (2, 8, 64, 2, 4, 0, True, False),
         (3, 12, 96, 2, 4, 4, False, False), (3, 12, 96, 2, 2, 64, True, True), (3, 12, 96, 2, 1, 5, False, False),
         (2, 8, 64, 3, 4, 0, True, False), (2, 8, 64, 3, 2, 3, False, True), (2, 8, 64, 3, 1, 0, True, False),
         (2, 8, 64, 1, 1, 0, False, False), (2, 8, 64, 1, 3, 2, True, True)]


@pytest.mark.parametrize("B,H,W,Cin,npass,blocks,carry_in,acc0", CASES)
def test_head_backward_in_the_product_epilogue_against_the_stored_product(B, H, W, Cin, npass, blocks, carry_in, acc0):
    """1 x 4 x 32: one tile, every border tap outside the image; 2 x 8 x 64: tiles adjacent both ways and across samples;
    3 x 12 x 96 (27 tiles) on 4 or 5 blocks (several tiles per block, uneven) and on 64 (more blocks than tiles).  1 pass (no
    carry), 2 and 4; Cin = 2, 3 and 1 (a one-pass case each: the stored-product path then runs k_head_bwd_mfma).  The slab starts as 7.0 everywhere under accumulate = 0 (rows no block owns must end as zero)
    or as 0.5 under accumulate = 1 (they must keep it)."""
    L = _lib.load()
    assert L.evf_head_dgrad_win_select(1, blocks) == 0
    assert L.evf_head_dgrad_win_fits(B, Cin, H, W, 1, ARCTAN, 1, 1, 0) == 1
    d = _inputs(B, Cin, H, W, npass, seed=100 * B + H + npass + Cin)
    ref_dw, ref_gl, ref_gt, ref_gv = _reference(d, B, Cin, H, W, npass, carry_in)
    old = _run(d, B, Cin, H, W, npass, False, carry_in, acc0)
    new = _run(d, B, Cin, H, W, npass, True, carry_in, acc0)
    assert torch.equal(old[0], new[0]), "dL/dv leaving the window"
    assert _err(old[0].double(), ref_gv) < 1e-5  # (the reference describes the same computation)
    nsl = L.evf_head_lif_bwd_wgrad_slabs(B, H, W)
    base = 0.5 * nsl if acc0 else 0.0
    lines = []
    for name, r, o, n in (("slab", ref_dw, old[1] - base, new[1] - base), ("g_leak", ref_gl, old[2][:32], new[2][:32]),
                          ("g_thresh", ref_gt, old[2][32:], new[2][32:])):
        eo, en = _err(o, r), _err(n, r)
        lines.append(f"{B}x{H}x{W} Cin{Cin} P{npass} blocks{blocks} carry{int(carry_in)} acc{int(acc0)} {name}: stored-product path {eo:.3e}  epilogue path {en:.3e}")
        print(lines[-1])
    rep = os.environ.get("EVF_HEAD_DGRAD_REPORT")
    if rep:
        with open(rep, "a") as f:
            f.write("\n".join(lines) + "\n")
    for name, r, o, n in (("slab", ref_dw, old[1] - base, new[1] - base), ("g_leak", ref_gl, old[2][:32], new[2][:32]),
                          ("g_thresh", ref_gt, old[2][32:], new[2][32:])):
        eo, en = _err(o, r), _err(n, r)
        assert eo < 1e-4, (name, eo)  # (the old path agrees with the reference at all: conv orientation, tap order)
        assert en <= 2.0 * eo, (name, en, eo)


def test_predicate_and_switch():
    L = _lib.load()
    assert L.evf_head_dgrad_win_select(-1, 0) == 0
    ok = (2, 2, 8, 64, 1, ARCTAN, 1, 1, 0)
    assert L.evf_head_dgrad_win_fits(*ok) == (0 if os.environ.get("EVF_HEAD_DGRAD_WIN", "1") == "0" else 1)
    assert L.evf_head_dgrad_win_select(1, 0) == 0
    assert L.evf_head_dgrad_win_fits(*ok) == 1
    assert L.evf_head_dgrad_win_fits(2, 3, 8, 64, 1, ARCTAN, 1, 1, 0) == 1
    for bad in ((2, 2, 37, 50, 1, ARCTAN, 1, 1, 0),   # ragged shape
                (2, 2, 8, 48, 1, ARCTAN, 1, 1, 0), (2, 2, 6, 64, 1, ARCTAN, 1, 1, 0),
                (2, 4, 8, 64, 1, ARCTAN, 1, 1, 0),     # Cin > 3
                (2, 2, 8, 64, 0, ARCTAN, 1, 1, 0),     # soft reset
                (2, 2, 8, 64, 3, ARCTAN, 1, 1, 0),     # an XLIF head (bit 1 of the flag)
                (2, 2, 8, 64, 1, SURROGATE_ID["superspike"], 1, 1, 0),
                (2, 2, 8, 64, 1, ARCTAN, 0, 1, 0),     # fp32 dL/d(current), no planes
                (2, 2, 8, 64, 1, ARCTAN, 1, 0, 0),     # one plane buffer for all passes
                (2, 2, 8, 64, 1, ARCTAN, 1, 1, 1)):    # deterministic mode
        assert L.evf_head_dgrad_win_fits(*bad) == 0, bad
    assert L.evf_head_dgrad_win_select(0, 0) == 0
    assert L.evf_head_dgrad_win_fits(*ok) == 0
    for B, H, W, Cin, *_ in CASES:  # switched off: no eligible shape of this file is served
        assert L.evf_head_dgrad_win_fits(B, Cin, H, W, 1, ARCTAN, 1, 1, 0) == 0
    # switched off / not eligible: the entry point refuses, nothing is launched
    B, Cin, H, W = 2, 2, 8, 64
    d = _inputs(B, Cin, H, W, 1, seed=3)
    x = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in d.items()}
    pb3 = torch.empty(54 * 1024, dtype=torch.uint8, device=DEV)
    nsl = L.evf_head_lif_bwd_wgrad_slabs(B, H, W)
    gv, slab, rows = torch.empty(B, H, W, C, device=DEV), torch.zeros(nsl, C * 18, device=DEV), torch.zeros(nsl, 64, device=DEV)
    rc = _lib.raw("evf_head_bwd_dgrad_win", P(x["planes"][0]), P(pb3), None, P(x["vs"][1]), None, None, P(x["xs"][0]), P(x["leak"]),
                  P(x["thresh"]), B, Cin, H, W, 1, ARCTAN, WIDTH, P(gv), P(rows[:, :32]), P(rows[:, 32:]), P(slab), 64 << 8)
    assert rc == ENOTSUP
    torch.cuda.synchronize()
    assert float(slab.abs().sum()) == 0.0 and float(rows.abs().sum()) == 0.0


class _EngineStep:
    """LIF-FireNet with a fixed upstream gradient as its loss (loss = sum flow * ups): one training window from the zero state,
    gradients into the optimizer's flat buffer (the window's sums reach it through ONE fixed-order launch, evf_grads_finalize --
    plain autograd gradients go through evf_reduce_slabs, whose float atomics differ from run to run).  step() syncs nowhere and
    allocates its inputs nowhere: it can be captured."""

    def __init__(self, shape, npass):
        from event_flow_amd import synthetic
        from event_flow_amd.dataloader.encodings import encode_event_list
        from event_flow_amd.models.model import LIFFireNet
        from event_flow_amd.train import FlatAdam

        B, H, W = shape
        self.shape, self.npass = shape, npass
        torch.manual_seed(7)
        cfg = {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
               "activations": ["arctanspike", "arctanspike"],
               "spiking_neuron": {"leak": [-4.0, 0.1], "thresh": [0.2, 0.05], "learn_leak": True, "learn_thresh": True, "hard_reset": True}}
        self.model = LIFFireNet(cfg).to(DEV)
        self.model.train()
        self.opt = FlatAdam(self.model, lr=1e-4, clip=100.0)
        self.opt.zero_grad()
        self.passes = [encode_event_list(torch.from_numpy(synthetic.event_list_batch(B, 300, H, W, 40 + k)).to(DEV), 2, (H, W))
                       for k in range(npass)]
        g = torch.Generator(device="cpu").manual_seed(1)
        self.ups = [torch.randn(B, 2, H, W, generator=g).to(DEV) for _ in range(npass)]
        self.tapes = None  # (filled by step(record=True): the tapes of the passes in backward order)

    def step(self, record=False):
        model, opt = self.model, self.opt
        model.reset_states()
        _lib.zero_(opt.flat_grad)
        model.defer_forward(True)
        try:
            flows = [model(d["event_voxel"], d["event_cnt"])["flow"][-1] for d in self.passes]
        finally:
            model.defer_forward(False)
        loss = sum((f * u).sum() for f, u in zip(flows, self.ups))
        opt.mark_grad_dirty()
        eng = model._engine
        if record:
            self.tapes, orig = [], eng._backward_pass

            def spy(win, tape, g_flow, is_first):
                self.tapes.append(tape)
                return orig(win, tape, g_flow, is_first)

            eng._backward_pass = spy
        model.defer_backward(True)
        try:
            loss.backward()
        finally:
            model.defer_backward(False)
            if record:
                del eng._backward_pass
        return loss.detach()

    def grads(self):
        out, off = {}, 0
        for k, p in self.model.named_parameters():
            if p.requires_grad:
                out[k] = self.opt.flat_grad[off:off + p.numel()].detach().cpu().clone().view(p.shape)
                off += p.numel()
        return out


def _engine_run(shape, npass, on):
    """One eager step of a fresh network with the switch as given -> (loss, gradients, the step object, calls of the new entry point)."""
    assert _lib.load().evf_head_dgrad_win_select(1 if on else 0, 0) == 0
    st = _EngineStep(shape, npass)
    calls, orig = [], _lib.call

    def counting(name, *a):
        if name == "evf_head_bwd_dgrad_win":
            calls.append(name)
        return orig(name, *a)

    _lib.call = counting
    try:
        loss = st.step(record=True)
    finally:
        _lib.call = orig
    torch.cuda.synchronize()
    return float(loss), st.grads(), st, len(calls)


def _head_reference(st):
    """float64 reference of the head layer's gradients of the step `st` just ran with the switch ON: from the head's tape, the
    input and layer 1's split planes of every pass as the engine kept them (G1's backward does not depend on the head's path:
    the same planes feed the stored-product path), through the reference of the direct cases."""
    eng = st.model._engine
    win = eng._last_window
    B, H, W = st.shape
    npass = st.npass
    assert len(st.tapes) == npass and len(win.gsl1) == npass
    heads = [tp["layers"][0] for tp in reversed(st.tapes)]  # forward order: (in_bits, v_prev, z_prev, v_out, ...)
    assert heads[0][1] is None and heads[0][2] is None  # (the window starts from the zero state)
    vs = [torch.zeros(B, H, W, C)] + [h[3].detach().cpu() for h in heads]
    zs = [torch.zeros(B, H, W, dtype=torch.int32)] + [h[2].detach().cpu() for h in heads[1:]]
    named = dict(st.model.named_parameters())
    d = {"leak": named["head.leak"].detach().cpu().reshape(C), "thresh": named["head.thresh"].detach().cpu().reshape(C),
         "wt": named["G1.ff.weight"].detach().cpu(), "xs": [tp["x_in"].detach().cpu() for tp in reversed(st.tapes)],
         "vs": vs, "zs": zs, "planes": [win.gsl1[k].detach().cpu() for k in range(npass)], "gv_in": None}
    dw, gl, gt, _ = _reference(d, B, 2, H, W, npass, False, width=eng._act_width(0))
    return {"head.ff.weight": dw.view(C, 2, 3, 3), "head.leak": gl.view(C, 1, 1), "head.thresh": gt.view(C, 1, 1)}


def test_engine_step_with_the_switch_on_and_off():
    """2 x 16 x 32, 3 passes (eligible).  The new path is taken with the switch on (three recorded cells, three plane buffers kept)
    and not with it off; loss and every gradient outside the head layer bit for bit; the head layer's gradients against float64:
    the epilogue path's largest error at most twice the stored-product path's."""
    shape, npass = (2, 16, 32), 3
    l_off, g_off, st_off, n_off = _engine_run(shape, npass, False)
    assert n_off == 0 and len(st_off.model._engine._last_window.gsl1) == 0
    l_on, g_on, st_on, n_on = _engine_run(shape, npass, True)
    assert n_on == npass and len(st_on.model._engine._last_window.gsl1) == npass and len(st_on.model._engine._last_window.gz0) == 0
    ref = _head_reference(st_on)
    l_off2, g_off2, _, _ = _engine_run(shape, npass, False)
    assert l_on == l_off == l_off2
    assert set(g_on) == set(g_off) and set(ref) == {k for k in g_on if k.startswith("head.")}
    for k in g_off:
        assert torch.equal(g_off[k], g_off2[k]), f"{k}: not reproducible with the switch off"
        if k in ref:
            assert float(ref[k].abs().max()) > 0
            eo, en = _err(g_off[k].double(), ref[k]), _err(g_on[k].double(), ref[k])
            print(f"engine 2x16x32 P3 {k}: stored-product path {eo:.3e}  epilogue path {en:.3e}")
            assert eo < 1e-4, (k, eo)
            assert en <= 2.0 * eo, (k, en, eo)
        else:
            assert torch.equal(g_on[k], g_off[k]), k


def test_engine_step_at_a_ragged_shape_is_untouched():
    """2 x 37 x 50 is not eligible: the switch changes nothing, every gradient bit for bit, the new entry point is never called."""
    l_off, g_off, _, n_off = _engine_run((2, 37, 50), 2, False)
    l_on, g_on, st, n_on = _engine_run((2, 37, 50), 2, True)
    assert n_off == 0 and n_on == 0 and len(st.model._engine._last_window.gsl1) == 0
    assert l_on == l_off and set(g_on) == set(g_off)
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    """The 2 x 16 x 32, 3-pass step with the switch on, captured after two eager steps and replayed: k_dgrad_head_win is a node of
    the graph (its buffers were allocated by the warm-up or belong to the capture's pool).  Loss and every gradient bit for bit."""
    assert _lib.load().evf_head_dgrad_win_select(1, 0) == 0
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        st = _EngineStep((2, 16, 32), 3)
        l1 = st.step()
        side.synchronize()
        g1 = st.grads()
        l2 = st.step(record=True)
        side.synchronize()
        g2 = st.grads()
        assert len(st.model._engine._last_window.gsl1) == 3  # (the epilogue path)
        assert float(l1) == float(l2) and all(torch.equal(g1[k], g2[k]) for k in g1)  # (eager steps repeat bit for bit)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):
            lg = st.step()
        st.opt.flat_grad.fill_(float("nan"))
        side.synchronize()
        for _ in range(2):
            graph.replay()
            side.synchronize()
            gg = st.grads()
            assert float(lg) == float(l2)
            for k in g2:
                assert torch.equal(gg[k], g2[k]), k
    cur.wait_stream(side)
