"""XLIF and ALIF FireNets (reference models/model.py:660-681; cells spiking_submodules.py:230-435, :660-875) on the recorded 32-channel
window kernels: the PLIF kernels with the pre-synaptic trace in the THRESHOLD (t0 + t1 * pt') instead of in the current
(include/evflow.h: bit 1 of the PLIF entry points' reset / accumulate flag).  Against the CPU oracle (pinned by the single-cell
goldens G6) and against the same network chained cell by cell on the general path."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from event_flow_amd import synthetic  # noqa: E402
from event_flow_amd.dataloader.encodings import encode_event_list  # noqa: E402
from event_flow_amd.loss import flow as hloss  # noqa: E402
from event_flow_amd.models.model import ALIFFireNet, XLIFFireNet  # noqa: E402
from event_flow_amd.train import FlatAdam, window_backward  # noqa: E402
from oracle import snn as osnn  # noqa: E402
from oracle.golden_parts import load_parts  # noqa: E402
from oracle import train as otrain  # noqa: E402

DEV = "cuda:0"
XLIF_NEURON = {"leak_v": [-4.0, 0.1], "leak_pt": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
               "learn_thresh": True, "hard_reset": True}
ALIF_NEURON = {"leak_v": [-4.0, 0.1], "leak_t": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
               "learn_thresh": True, "hard_reset": True}
NETS = {"XLIFFireNet": (XLIFFireNet, XLIF_NEURON, "leak_pt"), "ALIFFireNet": (ALIFFireNet, ALIF_NEURON, "leak_t")}


def N(t):
    return t.detach().cpu().numpy()


def cfg(neuron=XLIF_NEURON):
    return {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False,
            "mask_output": True, "activations": ["arctanspike", "arctanspike"], "spiking_neuron": dict(neuron)}


def loss_cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def _flip_census(model, ref_states):
    got = model.states
    nflip = sum(int((N(got[li][1]) != ref_states[li][1].numpy()).sum()) for li in range(7))
    return nflip, sum(ref_states[li][1].numel() for li in range(7))


@pytest.mark.parametrize("name", ["XLIFFireNet", "ALIFFireNet"])
@pytest.mark.parametrize("shape", [(2, 16, 20), (1, 37, 70)])
def test_xlif_firenet_on_the_fused_engine_vs_oracle(shape, name):
    """Three passes through plain autograd (one fused backward per pass, cell by cell): flows, every state tensor (potential, spikes,
    trace) and every parameter gradient -- t0, t1, both leaks, all weights -- against the oracle.  ALIF: the threshold trace is driven
    by the cell's own previous spikes, whose gradient reaches the pass before (the g_zx path of the fused backward kernels)."""
    B, H, W = shape
    cls, neuron, trace_leak = NETS[name]
    torch.manual_seed(5)
    model = cls(cfg(neuron)).to(DEV)
    assert model._fused() and model.compute_path[0] == "fused"
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for k, _ in model.named_parameters():
        params[k].requires_grad_(True)
    xs = [(torch.rand(B, 2, H, W) < 0.5).float() * torch.randint(1, 4, (B, 2, H, W)).float() for _ in range(3)]
    states = [None] * 7
    tot_ref, tot = 0, 0
    for x in xs:
        f_ref, states = osnn.firenet_forward(name, params, x, states, hard_reset=True)
        out = model(x.to(DEV), x.to(DEV))
        np.testing.assert_allclose(N(out["flow"][0]), f_ref.detach().numpy(), rtol=1e-4, atol=1e-7)
        tot_ref = tot_ref + (f_ref * torch.arange(f_ref.numel()).view(f_ref.shape).remainder(7)).sum()
        fl = out["flow"][0]
        tot = tot + (fl * torch.arange(fl.numel(), device=DEV).view(fl.shape).remainder(7)).sum()
    for li, st in enumerate(model.states):
        np.testing.assert_allclose(N(st), torch.stack(states[li]).detach().numpy(), rtol=1e-5, atol=2e-6)
    tot.backward()
    tot_ref.backward()
    for k, p in model.named_parameters():
        ref = params[k].grad
        ref = ref.numpy() if ref is not None else np.zeros(tuple(p.shape), np.float32)
        got = N(p.grad) if p.grad is not None else np.zeros_like(ref)
        denom = max(np.linalg.norm(ref), 1e-12)
        assert np.linalg.norm(got - ref) <= 2e-3 * denom + 1e-9, (k, np.linalg.norm(got - ref) / denom)
    for k in ("head.t1", "G1.t1", "R2b.t1", "head.t0", "G2." + trace_leak):  # (the adaptive threshold's own parameters carry signal)
        assert float(np.abs(N(dict(model.named_parameters())[k].grad)).max()) > 0, k


@pytest.mark.parametrize("name", ["XLIFFireNet", "ALIFFireNet"])
def test_xlif_recorded_window_matches_plain_autograd_the_general_path_and_the_oracle(monkeypatch, name):
    """One training window (4 passes, CM loss) three ways on the HIP side -- recorded (train.train_window: forward chains / diagonals,
    backward layer by layer with the window kernels), plain autograd on the fused kernels, and the general path (EVF_XLIF_FUSED=0:
    one conv + neuron kernel per cell) -- and through the oracle's train step: loss and the whole gradient."""
    B, n, H, W, P = 2, 900, 40, 70, 4
    cls, neuron, _ = NETS[name]
    XLIFFireNet = lambda c: cls(cfg(neuron))  # noqa: E731, N806  (the network under test, built from its own neuron configuration)
    torch.manual_seed(3)
    ref_model = XLIFFireNet(cfg()).to(DEV)
    sd = {k: v.detach().clone() for k, v in ref_model.state_dict().items()}
    passes = [encode_event_list(torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 900 + 10 * k)).to(DEV), 2, (H, W)) for k in range(P)]

    def grads_of(model, how):
        model.train()
        lossf = hloss.EventWarping(loss_cfg(H, W), DEV)
        if how == "recorded":
            opt = FlatAdam(model)  # (the parameters' .grad are views of its flat gradient buffer)
            opt.zero_grad()
            loss = window_backward(model, lossf, opt, passes)  # first half of train_window: passes, loss, backward -- no step
            g = {k: N(p.grad).copy() for k, p in model.named_parameters()}
        else:
            for d in passes:
                out = model(d["event_voxel"], d["event_cnt"])
                lossf.event_flow_association(out["flow"], d["event_list"], d["event_list_pol_mask"], d["event_mask"])
            loss = lossf()
            loss.backward()
            g = {k: N(p.grad).copy() for k, p in model.named_parameters()}
        return float(loss.detach()), g

    fused = XLIFFireNet(cfg()).to(DEV)
    fused.load_state_dict(sd)
    assert fused._fused()
    l_plain, g_plain = grads_of(fused, "plain")
    rec = XLIFFireNet(cfg()).to(DEV)
    rec.load_state_dict(sd)
    l_rec, g_rec = grads_of(rec, "recorded")
    monkeypatch.setenv("EVF_XLIF_FUSED", "0")
    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    gen = XLIFFireNet(cfg()).to(DEV)
    gen.load_state_dict(sd)
    assert not gen._fused() and gen.compute_path[0] == "general"
    l_gen, g_gen = grads_of(gen, "plain")
    monkeypatch.delenv("EVF_XLIF_FUSED")

    params = {k: v.detach().cpu().clone() for k, v in sd.items()}
    keys = [k for k, _ in ref_model.named_parameters()]  # (learn_thresh=True here: t0 / t1 are parameters, not the kind's default buffers)
    opasses = [{k: v.detach().cpu() for k, v in d.items()} for d in passes]
    l_ref, g_ref, _, ostates = otrain.train_step(name, params, keys, opasses, [None] * 7, (H, W), {"step": 0, "m": {}, "v": {}},
                                                 loss_cfg={"flow_regul_weight": 0.001, "mask_output": True},
                                                 model_cfg={"hard_reset": True})
    # same cells, same per-element arithmetic, other launch shapes: recorded == plain to the float atomics of the loss
    assert abs(l_rec - l_plain) <= 1e-6 * abs(l_plain)
    gn = float(np.sqrt(sum(float((g ** 2).sum()) for g in g_plain.values())))
    err = float(np.sqrt(sum(float(((g_rec[k] - g_plain[k]) ** 2).sum()) for k in g_plain)))
    assert err <= 2e-5 * gn, err / gn
    # general path and oracle: other summation orders in the convolutions -- borderline spikes may flip; the census decides the bar
    states = [None] * 7
    with torch.no_grad():
        for d in opasses:
            _, states = osnn.firenet_forward(name, params, d["event_cnt"], states, hard_reset=True)
    nflip, ntot = _flip_census(fused, states)
    assert nflip <= 1e-4 * ntot, (nflip, ntot)
    tol = 2e-3 if nflip == 0 else 5e-2
    np.testing.assert_allclose(l_plain, l_ref, rtol=1e-4 if nflip == 0 else 1e-3)
    np.testing.assert_allclose(l_gen, l_ref, rtol=1e-3)
    gref = float(np.sqrt(sum(float((g.numpy() ** 2).sum()) for g in g_ref.values())))
    for name, g in (("fused", g_plain), ("general", g_gen)):
        e = float(np.sqrt(sum(float(((g[k] - g_ref[k].numpy()) ** 2).sum()) for k in g)))
        assert e <= tol * gref, (name, e / gref, nflip)


@pytest.mark.parametrize("name", ["XLIFFireNet", "ALIFFireNet"])
def test_xlif_alif_hipgraph_replay_is_bitwise_the_eager_step_under_a_deterministic_loss(name):
    """The whole train step of a fused XLIF / ALIF FireNet replayed from hipGraphs (what bench.py's `firenet_family_at_c3_shape` times
    through train.GraphedWindowStep): device-side Adam counter, static state buffers incl. the trace, recorded forward and layer-major
    backward inside the capture.  As tests/test_gpu_network.py::test_hipgraph_replay_is_bitwise_the_eager_step_under_a_deterministic_loss
    for the LIF network: with a loss whose backward is deterministic (the contrast loss sums with float atomics: through it graph and
    eager steps of an alive network drift apart like two eager runs do, 1e-3 .. 1e-2 of the loss after a few steps) two eager + four
    replayed steps leave EXACTLY the parameters, Adam moments and recurrent states (potential, spikes, trace) of six eager steps."""
    from test_gpu_network import _LinearWindowLoss

    from event_flow_amd.train import train_window

    cls, neuron, _ = NETS[name]
    B, n, H, W, P = 2, 600, 32, 64, 3
    pool = [[torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 7100 + 100 * w + k)).to(DEV) for k in range(P)] for w in range(2)]
    gw = torch.Generator(device="cpu").manual_seed(9)
    wts = [(torch.randn(B, 2, H, W, generator=gw) * 0.02).to(DEV) for _ in range(P)]

    def make():
        torch.manual_seed(3)
        m = cls(cfg(neuron)).to(DEV)
        m.train()
        return m

    def step(model, lossf, opt, lists):
        passes = [encode_event_list(ev, 2, (H, W), want=("cnt", "mask", "pol")) for ev in lists]
        for d in passes:
            d["event_voxel"] = None
        return train_window(model, lossf, opt, passes)

    m1 = make()
    assert m1._fused()
    opt1 = FlatAdam(m1, lr=2e-4, clip=100.0, device_step=True)
    opt1.zero_grad()
    m1.use_static_states(True)
    l1 = _LinearWindowLoss(wts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(2):
            step(m1, l1, opt1, pool[i % 2])
        torch.cuda.synchronize()
        graphs = []
        for lists in pool:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                step(m1, l1, opt1, lists)
            graphs.append(g)
        for i in range(4):
            graphs[i % 2].replay()
        torch.cuda.synchronize()
    m2 = make()
    opt2 = FlatAdam(m2, lr=2e-4, clip=100.0, device_step=True)
    opt2.zero_grad()
    m2.use_static_states(True)
    l2 = _LinearWindowLoss(wts)
    for i in range(6):
        step(m2, l2, opt2, pool[i % 2])
    torch.cuda.synchronize()
    assert float(opt2.norm_ws[0].sqrt()) < 100.0  # no clipping: the (atomically summed) norm does not enter the update
    assert float(opt1.norm_ws[1]) == 6.0 and float(opt2.norm_ws[1]) == 6.0
    assert torch.equal(opt1.flat_param, opt2.flat_param)
    assert torch.equal(opt1.m, opt2.m) and torch.equal(opt1.v, opt2.v)
    for a, b in zip(m1.states, m2.states):
        assert torch.equal(a, b)
    sd0 = make().state_dict()
    assert any(float((p.detach() - sd0[k].to(DEV)).abs().max()) > 0 for k, p in m1.named_parameters() if k.endswith(("t0", "t1")))  # (the adaptive threshold trained)


# ------------------------------------------------------------------ the reference's own numbers (tests/golden/g7_{x,a}liffirenet_*)
LAYERS = ["head", "G1", "R1a", "R1b", "G2", "R2a", "R2b"]
# (fixture, network, path): hard-reset fixtures on the fused engine and -- EVF_XLIF_FUSED=0 -- on the general path; the soft-reset
# ones (the reference constructors' default) on the general path, which is what serves them
GOLDEN_FWD = [("g7_xliffirenet_train", "XLIFFireNet", "fused"), ("g7_aliffirenet_train", "ALIFFireNet", "fused"),
              ("g7_xliffirenet_train", "XLIFFireNet", "general"), ("g7_aliffirenet_train", "ALIFFireNet", "general"),
              ("g7_xliffirenet_soft", "XLIFFireNet", "soft"), ("g7_aliffirenet_soft", "ALIFFireNet", "soft")]
GOLDEN_TRAIN = GOLDEN_FWD[:2] + [("g7_xliffirenet_train", "XLIFFireNet", "recorded"), ("g7_aliffirenet_train", "ALIFFireNet", "recorded")] + GOLDEN_FWD[2:]


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _golden_model(g, name, path, monkeypatch):
    cls, neuron, _ = NETS[name]
    hard = bool(g["meta_hard_reset"])
    assert hard == (path != "soft")
    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    if path == "general":
        monkeypatch.setenv("EVF_XLIF_FUSED", "0")
    model = cls(cfg(dict(neuron, hard_reset=hard))).to(DEV)
    missing, unexpected = model.load_state_dict({k[len("param0_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param0_")})
    assert not missing and not unexpected  # the reference's state_dict keys load unchanged
    assert model.compute_path[0] == ("fused" if path in ("fused", "recorded") else "general"), model.compute_path
    assert model._fused() == (path in ("fused", "recorded"))
    return model


def _golden_passes(g):
    keys = ("event_cnt", "event_voxel", "event_list", "event_list_pol_mask", "event_mask")
    return [{k: G(g[f"p{i}_{k}"]) for k in keys} for i in range(int(g["meta_P"]))]


def _golden_thresh(g, i, ln):
    """The reference's per-element threshold of pass i, layer ln: t0.clamp_min(0.01) + t1.clamp_min(0) * trace'."""
    return np.maximum(g[f"param0_{ln}.t0"], np.float32(0.01))[None] + np.maximum(g[f"param0_{ln}.t1"], np.float32(0))[None] * g[f"p{i}_aux_{ln}"]


def _golden_forward(g, model, passes, tag):
    """The passes under no_grad against the reference's per-layer numbers with the bars of tests/test_gpu_network.py::
    test_forward_per_layer_and_flow: spikes equal wherever the reference's margin exceeds 1e-4; flips over ALL passes counted
    (<= 1e-5 of the elements: 7 of 774 144); while no spike has flipped v' and the trace rtol 1e-5 / atol 2e-6, flow rtol 1e-4.
    -> (flips, elements)."""
    nflip = ntot = 0
    worst_v = worst_t = worst_f = 0.0
    with torch.no_grad():
        for i, d in enumerate(passes):
            out = model(d["event_voxel"], d["event_cnt"], log=True)
            states = model.states
            for li, ln in enumerate(LAYERS):
                v_ref, z_ref, t_ref = g[f"p{i}_v_{ln}"], g[f"p{i}_z_{ln}"].astype(np.float32), g[f"p{i}_aux_{ln}"]
                v, z, tr = N(states[li][0]), N(states[li][1]), N(states[li][2])
                safe = np.abs(v_ref - _golden_thresh(g, i, ln)) > 1e-4
                nflip += int((z != z_ref).sum())
                ntot += z.size
                assert np.array_equal(z[safe], z_ref[safe]), (i, ln, int((z != z_ref)[safe].sum()))
                if nflip == 0:  # (a flipped borderline spike upstream legitimately changes everything downstream)
                    worst_v = max(worst_v, float((np.abs(v - v_ref) / (2e-6 + 1e-5 * np.abs(v_ref))).max()))
                    worst_t = max(worst_t, float((np.abs(tr - t_ref) / (2e-6 + 1e-5 * np.abs(t_ref))).max()))
                    np.testing.assert_allclose(v, v_ref, rtol=1e-5, atol=2e-6, err_msg=f"{i} {ln}")
                    np.testing.assert_allclose(tr, t_ref, rtol=1e-5, atol=2e-6, err_msg=f"{i} {ln} trace")
            if nflip == 0:
                f, f_ref = N(out["flow"][0]), g[f"p{i}_flow"]
                worst_f = max(worst_f, float((np.abs(f - f_ref) / (1e-7 + 1e-4 * np.abs(f_ref))).max()))
                np.testing.assert_allclose(f, f_ref, rtol=1e-4, atol=1e-7)
            assert set(out["activity"].keys()) == {"0:input", "1:head", "2:G1", "3:R1a", "4:R1b", "5:G2", "6:R2a", "7:R2b", "8:pred"}
    print(f"[{tag} forward] spike flips over all passes {nflip} of {ntot}; worst error as a fraction of its bar (while no spike had flipped): "
          f"v' {worst_v:.3f}, trace {worst_t:.3f}, flow {worst_f:.3f}")
    assert nflip <= 1e-5 * ntot, (nflip, ntot)
    return nflip, ntot


@pytest.mark.parametrize("fix,name,path", GOLDEN_FWD)
def test_golden_forward_per_layer_and_flow(monkeypatch, fix, name, path):
    """XLIF / ALIF FireNets against the REFERENCE's run (not the oracle's): per pass and layer the potential, the spikes and the
    threshold trace, and the flow.  The fixtures' model seeds were chosen for the largest minimum margin |v' - thresh|
    (6.6e-6 .. 1.4e-5, meta_min_margin), so a flip is possible and counted."""
    g = load_parts(fix)
    model = _golden_model(g, name, path, monkeypatch)
    model.eval()
    _golden_forward(g, model, _golden_passes(g), f"{fix} {path}")


@pytest.mark.parametrize("fix,name,path", GOLDEN_TRAIN)
def test_golden_train_step(monkeypatch, fix, name, path):
    """One training window (3 passes, contrast loss, backward, clip + Adam) against the reference's loss, gradient norm, 39 gradient
    tensors and updated parameters, with the bars tests/test_gpu_network.py::test_train_step_vs_golden holds LIF / PLIF to: loss
    2e-5, grad_norm 2e-4, every tensor 2e-4 of its own norm + 1e-6 of the whole gradient when the census over all passes found no
    spike flip (10x those when it did; at most 1e-5 of the spikes may flip).  `recorded`: FlatAdam + train.window_backward (the
    window kernels, layer by layer); `fused`: plain autograd on the fused kernels, pass by pass; `general` / `soft`: cell by cell."""
    g = load_parts(fix)
    trace_leak = NETS[name][2]
    gall = np.sqrt(sum(float((g[k].astype(np.float64) ** 2).sum()) for k in g.files if k.startswith("grad_") and k != "grad_norm"))
    np.testing.assert_allclose(gall, float(g["grad_norm"]), rtol=1e-5)
    for ln in LAYERS:  # the adaptive threshold's own parameters and both leaks carry signal in every layer: no bar below is vacuous
        for q in ("t0", "t1", "leak_v", trace_leak):
            # (more than the 1e-6 of the whole gradient every tensor's bar adds: a zero gradient would not pass for any of them)
            assert np.linalg.norm(g[f"grad_{ln}.{q}"]) > 1e-6 * gall, (ln, q, np.linalg.norm(g[f"grad_{ln}.{q}"]), gall)
    model = _golden_model(g, name, path, monkeypatch)
    model.train()
    passes = _golden_passes(g)
    nflip, ntot = _golden_forward(g, model, passes, f"{fix} {path}")  # the census (all passes); asserts <= 1e-5 of the elements
    model.reset_states()
    H, W = passes[0]["event_cnt"].shape[2:]
    lossf = hloss.EventWarping(loss_cfg(H, W), DEV)
    if path == "recorded":
        opt = FlatAdam(model, lr=2e-4, clip=100.0)
        opt.zero_grad()
        loss = window_backward(model, lossf, opt, passes)
    else:
        for d in passes:
            out = model(d["event_voxel"], d["event_cnt"])
            lossf.event_flow_association(out["flow"], d["event_list"], d["event_list_pol_mask"], d["event_mask"])
        loss = lossf()
        loss.backward()
    last = sum(int((N(model.states[li][1]) != g[f"p{len(passes) - 1}_z_{ln}"].astype(np.float32)).sum()) for li, ln in enumerate(LAYERS))
    assert last <= nflip, (last, nflip)  # (the window ran the spike trains the census saw)
    grads = {k: N(p.grad).copy() for k, p in model.named_parameters()}
    assert len(grads) == 39
    if path == "recorded":
        opt.step()
        gn = opt.grad_norm()
    else:
        gn = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 100.0))
        torch.optim.Adam(model.parameters(), lr=2e-4).step()
    newp = {k: N(v).copy() for k, v in model.state_dict().items()}
    loss = float(loss.detach())
    tight = nflip == 0
    worst = ("", 0.0)
    for k, got in grads.items():
        ref = g["grad_" + k]
        r = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-6 * gall))
        if r > worst[1]:
            worst = (k, r)
    e_all = np.sqrt(sum(float(((grads[k] - g["grad_" + k]).astype(np.float64) ** 2).sum()) for k in grads)) / gall
    print(f"[{fix} {path} train] spike flips over all passes {nflip} of {ntot}; loss rel {abs(loss - float(g['loss'])) / abs(float(g['loss'])):.2e}, "
          f"grad_norm rel {abs(gn - float(g['grad_norm'])) / float(g['grad_norm']):.2e}, whole gradient rel-L2 {e_all:.2e}, "
          f"worst tensor {worst[0]} {worst[1]:.2e}; " + ", ".join(
              f"{q} {max(float(np.linalg.norm(grads[f'{ln}.{q}'] - g[f'grad_{ln}.{q}']) / np.linalg.norm(g[f'grad_{ln}.{q}'])) for ln in LAYERS):.2e}"
              for q in ("t0", "t1", "leak_v", trace_leak)))
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=2e-5 if tight else 2e-4)
    np.testing.assert_allclose(gn, float(g["grad_norm"]), rtol=2e-4 if tight else 2e-3)
    for k, got in grads.items():
        ref = g["grad_" + k]
        denom = max(np.linalg.norm(ref), 1e-12)
        assert np.linalg.norm(got - ref) <= (2e-4 if tight else 2e-3) * denom + 1e-6 * gall, (k, np.linalg.norm(got - ref) / denom, nflip)
    for k, ref in ((k[len("param1_"):], g[k]) for k in g.files if k.startswith("param1_")):
        # the first Adam step moves every weight by ~lr*sign(g): weights whose gradient is at the fp32 noise floor may move the other
        # way (<= 2*lr apart); the bulk must agree
        d = np.abs(newp[k] - ref)
        assert d.max() <= 2 * 2e-4 + 1e-6, k
        assert np.mean(d > 2e-5) <= 0.02, (k, np.mean(d > 2e-5))


# ------------------------------------------------------------------ configurations the fused engine does not serve: general path
@pytest.mark.parametrize("name", ["XLIFFireNet", "ALIFFireNet"])
def test_voxel_input_xlif_alif_firenets_run_on_the_general_path_vs_oracle(monkeypatch, name):
    """`encoding: voxel, num_bins: 5` with the default (hard reset, arctan) XLIF / ALIF neuron: the fused engine's XLIF / ALIF head
    kernels take a two-channel input only, so FireNet._fused() must send the network to the general path -- it used to report
    compute_path == "fused" and raise EvflowError in its first backward.  Two passes, contrast loss, backward: flows, states and
    every parameter gradient against the oracle with the bars of tests/test_gpu_general.py::test_adaptive_threshold_firenets_vs_oracle."""
    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    B, n, H, W, P = 2, 400, 16, 20, 2
    cls, neuron, _ = NETS[name]
    torch.manual_seed(5)
    c = cfg(neuron)
    c.update(encoding="voxel", num_bins=5)
    model = cls(c).to(DEV)
    assert model.compute_path[0] == "general" and "5-channel input" in model.compute_path[1], model.compute_path
    assert not model._fused()
    model.train()
    passes = [encode_event_list(torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 4100 + 10 * k)).to(DEV), 5, (H, W)) for k in range(P)]
    assert tuple(passes[0]["event_voxel"].shape) == (B, 5, H, W)
    lossf = hloss.EventWarping(loss_cfg(H, W), DEV)
    flows = []
    for d in passes:
        out = model(d["event_voxel"], d["event_cnt"])
        flows.append(out["flow"][0])
        lossf.event_flow_association(out["flow"], d["event_list"], d["event_list_pol_mask"], d["event_mask"])
    loss = lossf()
    loss.backward()  # (raised EvflowError before)
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    keys = [k for k, _ in model.named_parameters()]
    leaves = {k: t.requires_grad_(k in keys) for k, t in params.items()}
    opasses = [{k: v.detach().cpu() for k, v in d.items()} for d in passes]
    l_ref, f_ref, st_ref = otrain.forward_window(name, leaves, opasses, [None] * 7, (H, W), loss_cfg={"flow_regul_weight": 0.001, "mask_output": True},
                                                 model_cfg={"hard_reset": True, "encoding": "voxel"})
    g_ref = torch.autograd.grad(l_ref, [leaves[k] for k in keys], allow_unused=True)
    for f, fr in zip(flows, f_ref):
        np.testing.assert_allclose(N(f), fr[0].detach().numpy(), rtol=1e-4, atol=1e-7)
    for li, st in enumerate(model.states):
        np.testing.assert_allclose(N(st), torch.stack(st_ref[li]).detach().numpy(), rtol=1e-5, atol=2e-6)
        assert float(st[1].detach().mean()) > 0.01, li  # (the layer spikes)
    np.testing.assert_allclose(float(loss.detach()), float(l_ref.detach()), rtol=1e-4)
    named = dict(model.named_parameters())
    worst = ("", 0.0)
    for k, ref in zip(keys, g_ref):
        ref = ref.numpy() if ref is not None else np.zeros(tuple(named[k].shape), np.float32)
        got = N(named[k].grad) if named[k].grad is not None else np.zeros_like(ref)
        denom = max(np.linalg.norm(ref), 1e-12)
        r = float(np.linalg.norm(got - ref) / denom)
        worst = max(worst, (k, r), key=lambda kr: kr[1])
        assert np.linalg.norm(got - ref) <= 2e-3 * denom + 1e-9, (k, r)
    print(f"[{name} voxel x5, general path] loss {float(loss.detach()):.6f} vs oracle {float(l_ref.detach()):.6f}; worst gradient tensor {worst[0]} {worst[1]:.2e}")
    assert float(np.abs(N(named["head.ff.weight"].grad)).max()) > 0 and tuple(named["head.ff.weight"].shape) == (32, 5, 3, 3)


_CHILD = """
import torch
from event_flow_amd import synthetic
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.loss import flow as hloss
from event_flow_amd.models import engine
from event_flow_amd.models.model import XLIFFireNet
from event_flow_amd.train import FlatAdam, train_window
assert not engine.PLIF_TRACE_FUSED
B, n, H, W, P = 2, 400, 16, 20, 2
torch.manual_seed(5)
model = XLIFFireNet({"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
                     "activations": ["arctanspike", "arctanspike"],
                     "spiking_neuron": {"leak_v": [-4.0, 0.1], "leak_pt": [-2.0, 0.1], "t0": [0.3, 0.05], "t1": [0.5, 0.1], "learn_leak": True,
                                        "learn_thresh": True, "hard_reset": True}}).to("cuda:0")
path = model.compute_path
assert path[0] == "general" and "EVF_PLIF_TRACE_FUSED" in path[1], path
assert not model._fused()
model.train()
before = {k: p.detach().clone() for k, p in model.named_parameters()}
opt = FlatAdam(model, lr=2e-4, clip=100.0)
opt.zero_grad()
lossf = hloss.EventWarping({"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
                            "model": {"mask_output": True}}, "cuda:0")
passes = [encode_event_list(torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 4100 + 10 * k)).to("cuda:0"), 2, (H, W)) for k in range(P)]
loss = float(train_window(model, lossf, opt, passes))
torch.cuda.synchronize()
moved = sum(int((p.detach() != before[k]).any()) for k, p in model.named_parameters())
assert loss == loss and moved == 39, (loss, moved)
print("TRAINED-ON-THE-GENERAL-PATH", loss, moved)
"""


def test_xlif_firenet_without_the_fused_trace_backward_trains_on_the_general_path():
    """EVF_PLIF_TRACE_FUSED=0 (read when models/engine.py is imported: a fresh child process): a default XLIF FireNet used to raise
    NotImplementedError when its engine was built; it trains one window on the general path."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVF_PLIF_TRACE_FUSED="0", EVF_PATH_NOTICE="0", PYTHONPATH=root, PYTHONNOUSERSITE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "TRAINED-ON-THE-GENERAL-PATH" in r.stdout, r.stdout[-2000:]
