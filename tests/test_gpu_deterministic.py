"""The deterministic contrast-maximisation loss on the GPU (evf_cm_loss_fwd_det / evf_cm_loss_bwd_det behind
loss.flow.set_deterministic): order independence bit for bit, parity with the goldens, with the default path and with a float64
evaluation, the refusals, and whole training steps that repeat bit for bit through the REAL loss."""

import copy
import os

import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden

pytestmark = pytest.mark.gpu

from event_flow_amd import _lib, synthetic  # noqa: E402
from event_flow_amd.dataloader.encodings import encode_event_list  # noqa: E402
from event_flow_amd.loss import flow as hloss  # noqa: E402
from event_flow_amd.models.model import LIFFireNet, XLIFFireNet  # noqa: E402
from event_flow_amd.train import FlatAdam, train_window  # noqa: E402
from oracle import loss as oloss  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVF_EINVAL, EVF_ENOTSUP = -22, -95


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def cfg(H, W, mask=True, overwrite=False, weight=0.001):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": weight, "overwrite_intermediate": overwrite},
            "model": {"mask_output": mask}}


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


# ------------------------------------------------------------------ windows
# (B, H, W, P, n, S, overwrite), then what is special.  The smallest shapes at which the new kernels can go wrong; rows of a stripe:
# 4096 / W capped at H, halved while above 8 (fewer than 512 blocks at these sizes) -- for both the forward and the backward stripes.
GEOMETRY = {
    "stripes": ((2, 24, 40, 3, 700, 1, False), {}),                      # rows 6: several full stripes, three dL/dflow maps per sample
    "ragged": ((3, 37, 53, 2, 900, 2, False), {}),                       # rows 4: short last stripe, ragged width, two scales
    "crowded-overwrite": ((2, 70, 41, 3, 500, 1, True), {"crowd": True}),  # one map per sample, events in rows H-6 .. H-2 only
    "widest": ((1, 3, 2048, 1, 600, 1, False), {}),                      # rows 2, the smallest the rule gives; 128 KiB / 64 KiB of LDS
    "four-scales": ((2, 32, 32, 2, 300, 4, False), {}),
    "empty-pass": ((2, 24, 40, 3, 300, 1, False), {"empty": 1}),         # pass 1 holds padding only (p = 0): its maps get no event term
    "leaving": ((2, 24, 40, 2, 600, 1, False), {"amp": 1.0}),            # flows large enough that events warp outside the image
}


def make_window(name, seed=5):
    (B, H, W, P, n, S, overwrite), opt = GEOMETRY[name]
    rng = np.random.default_rng(seed)
    amp = opt.get("amp", 0.1)
    win = dict(B=B, H=H, W=W, P=P, S=S, overwrite=overwrite, ev=[], pol=[], flows=[])
    for k in range(P):
        ev = synthetic.event_list_batch(B, n, H, W, 300 + k)
        if opt.get("crowd"):
            ev[:, :, 1] = np.floor(ev[:, :, 1] / H * 5.0) + (H - 6)
        if opt.get("empty") == k:
            ev[:, :, 3] = 0.0
        win["ev"].append(ev)
        win["pol"].append(np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], 2).astype(np.float32))
        win["flows"].append([rng.uniform(-amp, amp, size=(B, 2, H, W)).astype(np.float32) for _ in range(S)])
    return win


def permuted(win, seed=77):
    """the same SET of events: those of each pass of each sample in another order, polarity masks alike"""
    rng = np.random.default_rng(seed)
    out = dict(win, ev=[], pol=[])
    for ev, pol in zip(win["ev"], win["pol"]):
        ev2, pol2 = ev.copy(), pol.copy()
        for b in range(ev.shape[0]):
            p = rng.permutation(ev.shape[1])
            ev2[b], pol2[b] = ev[b, p], pol[b, p]
        out["ev"].append(ev2)
        out["pol"].append(pol2)
    return out


def run_loss(win):
    """EventWarping in the mode in force -> (loss, gradients by pass and scale; the overwritten window: of its last pass)"""
    B, H, W, P, S = (win[k] for k in "BHWPS")
    lossf = hloss.EventWarping(cfg(H, W, overwrite=win["overwrite"]), DEV)
    fls = []
    for k in range(P):
        fl = [G(f).requires_grad_(True) for f in win["flows"][k]]
        fls.append(fl)
        lossf.event_flow_association(fl, G(win["ev"][k]), G(win["pol"][k]), torch.ones(B, 1, H, W, device=DEV))
    if win["overwrite"]:
        lossf.overwrite_intermediate_flow(fls[-1])
    val = lossf()
    val.backward()
    torch.cuda.synchronize()
    grads = [N(f.grad) if f.grad is not None else None for fl in fls for f in fl]
    return N(val).copy(), grads


def cabi_forward_det(win):
    """evf_cm_loss_fwd_det called directly -> (images, stats, loss)"""
    B, H, W, P, S = (win[k] for k in "BHWPS")
    lib = _lib.load()
    Pm = 1 if win["overwrite"] else P
    maps = [win["flows"][-1]] if win["overwrite"] else win["flows"]
    fl = G(np.stack([np.stack([maps[p][s] for p in range(Pm)]) for s in range(S)]))  # [S,Pm,B,2,H,W]
    ev, pol = G(np.concatenate(win["ev"], 1)), G(np.concatenate(win["pol"], 1))
    M = ev.shape[1]
    ev_pass = G(np.repeat(np.arange(P, dtype=np.int32), [e.shape[1] for e in win["ev"]]))
    mask = torch.ones(B, Pm, H, W, device=DEV)
    images = torch.full((S, B, 8, H, W), float("nan"), device=DEV)
    stats = torch.full((S, B, 2, 2), float("nan"), device=DEV)
    part = torch.empty(S, lib.evf_cm_smooth_blocks(B, Pm, H, W), device=DEV)
    loss = torch.empty(1, device=DEV)
    nws = lib.evf_cm_loss_ws_det(S, B, M, H, W)
    assert nws > 0
    ws = torch.full((nws,), float("nan"), device=DEV)  # (the call clears what it accumulates into)
    flags = 1 | (2 if win["overwrite"] else 0) | 4
    _lib.call("evf_cm_loss_fwd_det", fl.data_ptr(), ev.data_ptr(), pol.data_ptr(), ev_pass.data_ptr(), mask.data_ptr(), S, P, B, M, H, W,
              float(max(H, W)), 0.001, flags, images.data_ptr(), stats.data_ptr(), part.data_ptr(), loss.data_ptr(), ws.data_ptr(), nws)
    torch.cuda.synchronize()
    return N(images), N(stats), N(loss)


_CACHE = {}


def results(name):
    """every window once per mode: (default, deterministic) -> (loss, grads); shared by the cases below, never modified"""
    if name not in _CACHE:
        win = make_window(name)
        before = _lib.deterministic()
        try:
            _lib.set_deterministic(False)
            plain = run_loss(win)
            _lib.set_deterministic(True)
            det = run_loss(win)
        finally:
            _lib.set_deterministic(before)
        _CACHE[name] = (win, plain, det)
    return _CACHE[name]


# ------------------------------------------------------------------ A: order independence, bit for bit
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_a_results_do_not_depend_on_the_order_of_the_events(name, det_on):
    """The real statement of the mode: the SAME SET of events in another order within every pass of every sample gives the same bits
    -- the images and statistics (read through the C ABI), the loss, and every flow gradient.  (The default path's float atomics do
    not have this property; the parent has no such entry points.)"""
    win, _, (loss, grads) = results(name)
    other = permuted(win)
    assert any(not np.array_equal(a, b) for a, b in zip(win["ev"], other["ev"]))
    im0, st0, l0 = cabi_forward_det(win)
    im1, st1, l1 = cabi_forward_det(other)
    assert np.isfinite(im0).all() and np.isfinite(st0).all() and np.abs(im0).sum() > 0
    assert np.array_equal(im0, im1)
    assert np.array_equal(st0, st1)
    assert np.array_equal(l0, l1) and np.array_equal(l0.reshape(()), loss)  # (and the Python path is that call)
    loss2, grads2 = run_loss(other)
    assert np.array_equal(loss, loss2)
    assert len(grads) == len(grads2)
    for a, b in zip(grads, grads2):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    assert any(g is not None and np.abs(g).max() > 0 for g in grads)
    if name == "leaving":  # (events did leave: less mass in the event images than events with a polarity)
        npol = sum(float(p.sum()) for p in win["pol"])
        assert float(im0[:, :, 0:2].sum()) < 0.9 * npol


# ------------------------------------------------------------------ B: the golden cases at the project's bars
def _run_golden_case(g, c, H, W):
    tag = c["tag"]
    lossf = hloss.EventWarping(cfg(H, W, c["mask"], c["overwrite"]), DEV)
    flows = []
    for k in range(c["P"]):
        fl = [G(g[f"{tag}_p{k}_flow{s}"]).requires_grad_(True) for s in range(c["scales"])]
        flows.append(fl)
        lossf.event_flow_association(fl, G(g[f"{tag}_p{k}_event_list"]), G(g[f"{tag}_p{k}_event_list_pol_mask"]), G(g[f"{tag}_p{k}_event_mask"]))
    if c["overwrite"]:
        lossf.overwrite_intermediate_flow(flows[-1])
    val = lossf()
    val.backward()
    return val, flows


def _golden_bars():
    g = load_golden("g4_event_warping")
    H, W = (int(v) for v in g["res"])
    for c in golden_cases(g):
        val, flows = _run_golden_case(g, c, H, W)
        np.testing.assert_allclose(float(val.detach()), float(g[c["tag"] + "_loss"]), rtol=1e-5, err_msg=str(c))
        for k in range(c["P"]):
            for s in range(c["scales"]):
                ref = g[f"{c['tag']}_p{k}_gflow{s}"]
                got = flows[k][s].grad
                got = N(got) if got is not None else np.zeros_like(ref)
                scale = max(np.abs(ref).max(), 1e-12)
                assert np.abs(got - ref).max() <= 1e-3 * scale + 1e-9, (c, k, s, np.abs(got - ref).max(), scale)
                assert np.linalg.norm(got - ref) <= 2e-4 * np.linalg.norm(ref) + 1e-9, (c, k, s)


def test_b_golden_loss_and_gradients_in_deterministic_mode(det_on):
    """g4_event_warping (the reference's own numbers) at the bars of test_event_warping_golden_loss_and_grad: loss rtol 1e-5,
    gradient max-norm 1e-3 of the scale + 1e-9, gradient L2 2e-4."""
    _golden_bars()


# ------------------------------------------------------------------ C: deterministic against the default path
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_c_deterministic_path_matches_the_default_path(name):
    """The same per-event terms summed another way: gradients within 1e-5 of the maximum (the path-against-path bar of
    test_event_gradient_stripes_match_atomics_on_ragged_shapes), the loss within rtol 1e-5."""
    _, (lp, gp), (ld, gd) = results(name)
    np.testing.assert_allclose(ld, lp, rtol=1e-5)
    for a, b in zip(gp, gd):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.abs(a - b).max() <= 1e-5 * max(np.abs(a).max(), 1e-12), (name, np.abs(a - b).max(), np.abs(a).max())


def test_c_default_stripe_images_equal_the_exact_sum_images(monkeypatch):
    """k_cm_splat_lds against k_cm_splat_det bit for bit where the sums are fractional.  Dyadic inputs (event times in 1/8, flows
    in 1/64 with flow_scaling 128, polarities +-1 on a few shared columns: warped coordinates in 1/4, terms in 2^-7, 1800 of them
    per sample), so every partial sum of an image is exact in fp32 and the float atomics have no order to depend on: the images
    must be EQUAL.  B = 2, 37 x 53, two passes of 900 events, two scales: stripes of 4 rows and a last one of 1 in both forms.
    The default's statistics are float atomics over non-dyadic squares: the losses agree to rtol 1e-6, not bitwise."""
    B, H, W, P, n, S = 2, 37, 53, 2, 900, 2
    monkeypatch.setattr(hloss, "CM_LDS_MIN_EVENTS", 0)  # (7200 event-scale pairs: the default call takes the stripe kernel all the same)
    rng = np.random.default_rng(23)
    evs, pols, flows = [], [], []
    for _ in range(P):
        ev = np.empty((B, n, 4), np.float32)
        ev[:, :, 0] = rng.integers(0, 9, size=(B, n)) / 8.0
        ev[:, :, 1] = rng.integers(0, H, size=(B, n))
        ev[:, :, 2] = rng.integers(0, 12, size=(B, n)) + 20
        ev[:, :, 3] = rng.integers(0, 2, size=(B, n)) * 2 - 1
        evs.append(ev)
        pols.append(np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], 2).astype(np.float32))
        flows.append([(rng.integers(-12, 13, size=(B, 2, H, W)) / 64.0).astype(np.float32) for _ in range(S)])
    got = {}
    before = _lib.deterministic()
    try:
        for on in (False, True):
            _lib.set_deterministic(on)
            lossf = hloss.EventWarping(cfg(H, W), DEV, flow_scaling=128)
            for k in range(P):
                lossf.event_flow_association([G(f).requires_grad_(True) for f in flows[k]], G(evs[k]), G(pols[k]),
                                             torch.ones(B, 1, H, W, device=DEV))
            val = lossf()
            got[on] = (N(val.grad_fn.saved_tensors[1]).copy(), N(val).copy())
    finally:
        _lib.set_deterministic(before)
    (im_p, loss_p), (im_d, loss_d) = got[False], got[True]
    assert im_p.shape == (S, B, 8, H, W) and np.isfinite(im_p).all()
    assert (im_d[:, :, :, H - 1] != 0).any()  # (the short last stripe holds terms)
    assert np.array_equal(im_p, im_d)
    np.testing.assert_allclose(loss_p, loss_d, rtol=1e-6)


# ------------------------------------------------------------------ accuracy against float64
def _float64(win):
    B, H, W, P, S = (win[k] for k in "BHWPS")
    ow = oloss.Window((H, W))
    fls = []
    for k in range(P):
        fl = [torch.from_numpy(f.astype(np.float64)).requires_grad_(True) for f in win["flows"][k]]
        fls.append(fl)
        ow.add(fl, torch.from_numpy(win["ev"][k].astype(np.float64)), torch.from_numpy(win["pol"][k].astype(np.float64)),
               torch.ones(B, 1, H, W, dtype=torch.float64))
    ref = oloss.event_warping_loss(ow, max(H, W), 0.001)
    ref.backward()
    return float(ref.detach()), [f.grad.numpy() for fl in fls for f in fl]


def _errors(loss, grads, ref_loss, ref_grads):
    """case B's norms over all flow gradients of the window: loss relative, gradient max-norm over the scale, gradient L2 relative"""
    got = np.concatenate([g.ravel() for g in grads]).astype(np.float64)
    ref = np.concatenate([g.ravel() for g in ref_grads])
    return (abs(float(loss) - ref_loss) / abs(ref_loss), np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12),
            np.linalg.norm(got - ref) / np.linalg.norm(ref))


def test_accuracy_against_float64_is_that_of_the_default_path():
    """Loss and gradients of two windows evaluated by the oracle in float64; the default and the deterministic path are fp32
    evaluations of identical per-event terms and differ in how the sums round, so the deterministic path's error may be at most
    twice the default path's error of this same run, plus 1e-9.  The figures go to profiles/deterministic_loss_report.txt."""
    lines = ["deterministic contrast loss against a float64 evaluation (oracle/loss.py); errors of the default (float atomics) and the",
             "deterministic path: loss relative, gradient max-norm over max|ref|, gradient L2 relative", ""]
    bad = []
    for name in ("stripes", "ragged"):
        win, (lp, gp), (ld, gd) = results(name)
        ref_loss, ref_grads = _float64(win)
        ep, ed = _errors(lp, gp, ref_loss, ref_grads), _errors(ld, gd, ref_loss, ref_grads)
        shape = GEOMETRY[name][0]
        lines.append(f"{name} (B,H,W,P,n,S,overwrite)={shape}")
        lines.append(f"  default        loss {ep[0]:.3e}  grad max {ep[1]:.3e}  grad l2 {ep[2]:.3e}")
        lines.append(f"  deterministic  loss {ed[0]:.3e}  grad max {ed[1]:.3e}  grad l2 {ed[2]:.3e}")
        print("\n".join(lines[-3:]))
        for what, p, d in zip(("loss", "grad max", "grad l2"), ep, ed):
            if not d <= 2.0 * p + 1e-9:
                bad.append((name, what, d, p))
    with open(os.path.join(ROOT, "profiles", "deterministic_loss_report.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not bad, bad


# ------------------------------------------------------------------ refusals
def test_refusals_precede_any_launch(det_on):
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    ti = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, pi = t.data_ptr(), ti.data_ptr()
    st = _lib.stream_ptr()

    def fwd(P, M, H, W, ws=p, n=1 << 40, S=1, B=1):
        return lib.evf_cm_loss_fwd_det(p, p, p, pi, p, S, P, B, M, H, W, 64.0, 0.001, 5, p, p, p, p, ws, n, st)

    def bwd(P, M, H, W, ws=p, n=1 << 40, S=1, B=1):
        return lib.evf_cm_loss_bwd_det(p, p, p, pi, p, S, P, B, M, H, W, 64.0, 0.001, 5, p, p, p, p, p, ws, n, st)

    # M * P beyond the admitted range (k < 32): tiny buffers, the check precedes any launch
    assert fwd(1 << 10, 1 << 20, 8, 8) == EVF_ENOTSUP and bwd(1 << 10, 1 << 20, 8, 8) == EVF_ENOTSUP
    assert lib.evf_cm_loss_bwd_ws_det(1, 1 << 10, 1, 1 << 20, 8, 8, 5) == 0 and lib.evf_cm_loss_ws_det(1, 1, 1 << 30, 8, 8) == 0
    # a row of 2049 pixels
    assert fwd(1, 16, 4, 2049) == EVF_ENOTSUP and bwd(1, 16, 4, 2049) == EVF_ENOTSUP
    assert lib.evf_cm_loss_ws_det(1, 1, 16, 4, 2049) == 0 and lib.evf_cm_loss_bwd_ws_det(1, 1, 1, 16, 4, 2049, 5) == 0
    assert lib.evf_cm_loss_ws_det(1, 1, 16, 4, 2048) > 0 and lib.evf_cm_loss_bwd_ws_det(1, 1, 1, 16, 4, 2048, 5) > 0
    # a null or short workspace
    nf, nb = lib.evf_cm_loss_ws_det(1, 1, 16, 8, 8), lib.evf_cm_loss_bwd_ws_det(1, 1, 1, 16, 8, 8, 5)
    assert nf > 0 and nb > 0
    assert fwd(1, 16, 8, 8, ws=None) == EVF_EINVAL and bwd(1, 16, 8, 8, ws=None) == EVF_EINVAL
    assert fwd(1, 16, 8, 8, n=nf - 1) == EVF_EINVAL and bwd(1, 16, 8, 8, n=nb - 1) == EVF_EINVAL
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0 and int(ti.abs().sum()) == 0  # nothing ran
    # the Python path says why, and does not fall back to the atomics
    B, H, W, n = 1, 2, 2049, 50
    lossf = hloss.EventWarping(cfg(H, W), DEV)
    ev = G(synthetic.event_list_batch(B, n, H, W, 1))
    pol = torch.stack([(ev[:, :, 3] > 0).float(), (ev[:, :, 3] < 0).float()], 2).contiguous()
    lossf.event_flow_association([torch.zeros(B, 2, H, W, device=DEV, requires_grad=True)], ev, pol, torch.ones(B, 1, H, W, device=DEV))
    with pytest.raises(_lib.EvflowError, match="2048"):
        lossf()


# ------------------------------------------------------------------ the step
LIF_NEURON = {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}
XLIF_NEURON = {"leak_v": [-4.0, 0.1], "leak_pt": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
               "learn_thresh": True, "hard_reset": True}


def _model_cfg(neuron):
    return {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False,
            "mask_output": True, "activations": ["arctanspike", "arctanspike"], "spiking_neuron": dict(neuron)}


def _steps(cls, neuron, runs):
    """`runs`: list of "eager" / "graph".  Every run starts from the same state_dict and trains three windows through the real
    EventWarping (static states, recorded forward and backward, device-side step counter); "graph": the third window is captured
    into a hipGraph and replayed instead of launched.  -> per run (parameters, Adam m, Adam v, recurrent states)."""
    B, n, H, W, P = 2, 400, 32, 40, 3
    pool = [[G(synthetic.event_list_batch(B, n, H, W, 7300 + 100 * w + k)) for k in range(P)] for w in range(3)]
    torch.manual_seed(3)
    first = cls(_model_cfg(neuron)).to(DEV)
    with torch.no_grad():
        for k, p in first.named_parameters():
            if k.endswith("thresh"):
                p.mul_(0.25)  # (an alive network: spikes in every layer)
    sd0 = copy.deepcopy(first.state_dict())

    def step(model, lossf, opt, lists):
        passes = [encode_event_list(ev, 2, (H, W), want=("cnt", "mask", "pol")) for ev in lists]
        for d in passes:
            d["event_voxel"] = None
        return train_window(model, lossf, opt, passes)

    out = []
    for kind in runs:
        m = cls(_model_cfg(neuron)).to(DEV)
        m.load_state_dict(sd0)
        m.train()
        opt = FlatAdam(m, lr=2e-4, clip=100.0, device_step=True)
        opt.zero_grad()
        start = opt.flat_param.clone()
        m.use_static_states(True)
        lossf = hloss.EventWarping(cfg(H, W), DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            losses = [step(m, lossf, opt, pool[w]) for w in range(2)]
            torch.cuda.synchronize()
            if kind == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    step(m, lossf, opt, pool[2])
                g.replay()
            else:
                losses.append(step(m, lossf, opt, pool[2]))
            torch.cuda.synchronize()
        assert float(opt.norm_ws[1]) == 3.0 and all(np.isfinite(float(x)) for x in losses)
        assert float((opt.flat_param - start).abs().max()) > 0  # (it trained)
        out.append((opt.flat_param.clone(), opt.m.clone(), opt.v.clone(), [s.clone() for s in m.states]))
        opt.close()
    return out


def _same(a, b):
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


def test_training_steps_repeat_bit_for_bit_through_the_real_loss(det_on):
    """LIFFireNet, 2 x 32 x 40, three passes of 400 events, FlatAdam, the REAL EventWarping: (a) two independent runs of three
    windows from one state_dict, (b) the third window replayed from a captured hipGraph against the same window launched eagerly --
    parameters, both Adam moments and all recurrent states torch.equal."""
    eager1, eager2, graph = _steps(LIFFireNet, LIF_NEURON, ["eager", "eager", "graph"])
    _same(eager1, eager2)
    _same(eager1, graph)


def test_xlif_graph_replay_is_the_eager_step_through_the_real_loss(det_on):
    eager, graph = _steps(XLIFFireNet, XLIF_NEURON, ["eager", "graph"])
    _same(eager, graph)


# ------------------------------------------------------------------ switch off
def test_switch_off_routes_to_the_default_path():
    """With the switch off the loss takes the default entry points: it still meets case B's bars, two calls on identical inputs
    agree bit for bit in the images wherever those are integer-valued (zero flow: every event image pixel is an exact count), and
    the deterministic entry points are not what ran (profile brackets see evf_cm_loss_fwd / evf_cm_loss_bwd only)."""
    before = _lib.deterministic()
    _lib.set_deterministic(False)
    try:
        _golden_bars()
        (B, H, W, P, n, S, _), _ = GEOMETRY["ragged"]
        lib = _lib.load()
        ev = G(np.concatenate([synthetic.event_list_batch(B, n, H, W, 300 + k) for k in range(P)], 1))
        pol = torch.stack([(ev[:, :, 3] > 0).float(), (ev[:, :, 3] < 0).float()], 2).contiguous()
        ev_pass = G(np.repeat(np.arange(P, dtype=np.int32), n))
        fl = torch.zeros(S, P, B, 2, H, W, device=DEV)
        ims = []
        for _ in range(2):
            images = torch.empty(S, B, 8, H, W, device=DEV)
            stats, loss = torch.empty(S, B, 2, 2, device=DEV), torch.empty(1, device=DEV)
            part = torch.empty(S, lib.evf_cm_smooth_blocks(B, P, H, W), device=DEV)
            _lib.call("evf_cm_loss_fwd", fl.data_ptr(), ev.data_ptr(), pol.data_ptr(), ev_pass.data_ptr(), None, S, P, B, P * n, H, W,
                      float(max(H, W)), 0.001, 4, images.data_ptr(), stats.data_ptr(), part.data_ptr(), loss.data_ptr(), None)
            torch.cuda.synchronize()
            ims.append(N(images))
        counts = ims[0][:, :, [0, 1, 4, 5]]
        assert np.array_equal(counts, np.round(counts)) and counts.sum() == 2 * S * float(pol.sum())
        assert np.array_equal(counts, ims[1][:, :, [0, 1, 4, 5]])
        win = make_window("stripes")
        _lib.profile_start(["evf_cm_loss_fwd", "evf_cm_loss_bwd", "evf_cm_loss_fwd_det", "evf_cm_loss_bwd_det"])
        run_loss(win)
        seen = {k[0] for k, v in _lib.profile_stop().items() if v}
        assert seen == {"evf_cm_loss_fwd", "evf_cm_loss_bwd"}
        _lib.set_deterministic(True)
        _lib.profile_start(["evf_cm_loss_fwd", "evf_cm_loss_bwd", "evf_cm_loss_fwd_det", "evf_cm_loss_bwd_det"])
        run_loss(win)
        seen = {k[0] for k, v in _lib.profile_stop().items() if v}
        assert seen == {"evf_cm_loss_fwd_det", "evf_cm_loss_bwd_det"}
    finally:
        _lib.set_deterministic(before)
