"""CPU only: what tests/test_gpu_zoo_ops.py asserts on the device stands on this.  (1) The float64 references of
tests/zoo_ops_ref.py agree with independent formulations: torch's float64 functional ops and autograd.  (2) The float32
emulations stay inside the bounds of the GPU test on its own inputs, and the exact cases are exact.  (3) The figures of rule 3
are measured here, printed, and equal to zoo_ops_ref.MEASURED.  (4) Every mutant of zoo_ops_ref.MUTANTS violates the GPU
test's assertion on at least one listed case."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import zoo_det_ref as ZD
import zoo_ops_ref as R

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.array(a, F64))  # noqa: E731


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * (1 + np.abs(b))), float(np.max(np.abs(a - b)))


def emulated(family, case, mut=None):
    inp = R.make(family, case)
    return R.fractions(R.expect(family, case, inp), R.outputs(R.run(family, case, inp, F32, mut)))


# ------------------------------------------------------------------------------------------------- (2), (3): bounds, MEASURED
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_stays_inside_the_bounds_of_the_gpu_test(family):
    """Rules 1 and 2: fraction <= 1 (rule 1: 0).  Rule 3: the emulation is what MEASURED was taken from: <= 1 / 4 of the bound."""
    for case in R.CASES[family]:
        inp = R.make(family, case)
        exp = R.expect(family, case, inp)
        for name, f in R.fractions(exp, R.outputs(R.run(family, case, inp, F32))).items():
            assert f <= (0.25 if exp[name].rule == 3 else 1.0), (family, case, name, f)
        if all(o.rule == 1 for o in exp.values()):  # the exact cases are exact on the reference alone
            assert all(f == 0.0 for f in R.fractions(exp, R.outputs(R.run(family, case, inp, F64))).values()), (family, case)


def test_measured_figures_are_the_stored_ones():
    seen = {}
    for family in R.FAMILIES:
        for case in R.CASES[family]:
            inp = R.make(family, case)
            exp = R.expect(family, case, inp)
            for name, f in R.fractions(exp, R.outputs(R.run(family, case, inp, F32))).items():
                if exp[name].rule == 3:
                    seen[exp[name].key] = max(seen.get(exp[name].key, 0.0), f * exp[name].factor())
    print("measured, units of 2^-24 * scale: " + "  ".join(f"{k} {v:.4g}" for k, v in sorted(seen.items())))
    assert set(seen) == set(R.MEASURED)
    for k, v in seen.items():
        assert 0.9 * R.MEASURED[k] <= v <= R.MEASURED[k], (k, v, R.MEASURED[k])


def test_weight_norm_rows_clear_the_float32_range_by_a_margin():
    """Whether a row's sum of squares overflows float32 must not hang on the order of the additions; and the 1e-18 row's squares
    are normal numbers."""
    for case in R.WN_CASES:
        v = np.asarray(R.make("wn_fwd", case)["v"], F64)
        ss = (v ** 2).sum(1)
        assert np.all((ss < 0.9 * R.FLT_MAX) | (ss > 1.1 * R.FLT_MAX)), (case, ss)
        assert np.all(v ** 2 > 2.0 ** -126)
    assert any(R.wn_overflows(R.make("wn_fwd", c)["v"]).any() for c in R.WN_CASES)
    assert any(c[0] >= 3 and not R.wn_overflows(R.make("wn_fwd", c)["v"])[2] for c in R.WN_CASES)  # 1e18 rows that stay finite


def test_torch_float32_weight_norm_overflows_as_the_expectation_says():
    """The parity rows of zoo_ops_ref._expect_wn_fwd / _bwd: torch's own float32 op gives nrm = inf, w = 0, zero gradients."""
    case = (3, 4608)
    inp = R.make("wn_bwd", case)
    v = torch.from_numpy(np.array(inp["v"])).requires_grad_()
    g = torch.from_numpy(np.array(inp["g"])).reshape(-1, 1).requires_grad_()
    w, nrm = torch._weight_norm_interface(v, g, 0)
    w.backward(torch.from_numpy(np.array(inp["gw"])))
    exp_f, exp_b = R.expect("wn_fwd", case, inp), R.expect("wn_bwd", case, inp)
    assert np.isinf(exp_f["nrm"].ref[2]) and float(nrm[2]) == np.inf
    assert not exp_f["w"].ref[2].any() and not bool(w[2].any())
    assert not exp_b["gv"].ref[2].any() and not bool(v.grad[2].any()) and float(g.grad[2]) == 0.0 and exp_b["gg"].ref[2] == 0.0
    # ... and the finite rows, the 1e-18 one included, as float64 has them
    close(w[:2].detach().numpy(), exp_f["w"].ref[:2], 1e-5)
    close(v.grad[:2].numpy(), exp_b["gv"].ref[:2] , 1e-4)


# ------------------------------------------------------------------------------------------------------------- (4): mutants
def _chan_mutant_fails():
    for G, npg, C in R.CHAN_CASES:
        x, y, center, scale = R.chan_int_inputs(G, npg, C, 0)
        xm, ym = R.chan_drop_tail(x, y, G, npg, C)
        for mode in range(3):
            ref = ZD.chan_ref64(x, y, center, scale, mode, G, npg, C)[0]
            got = ZD.chan_ref64(xm, ym, center, scale, mode, G, npg, C)[0]
            if not R.bits_equal(got, ref).all():
                return True
    return False


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_fails_the_gpu_assertion_somewhere(mut):
    if mut == "reduction_drops_tail":
        assert _chan_mutant_fails()
        return
    failed = [(family, case) for family in R.MUTANT_FAMILIES[mut] for case in R.CASES[family]
              if max(emulated(family, case, mut).values()) > 1.0]
    print(f"{mut}: fails {len(failed)} cases, the first {failed[:1]}")
    assert failed, mut


def test_chan_reduce_exact_inputs_are_exact_and_the_emulation_inside_rule_2():
    for G, npg, C in R.CHAN_CASES:
        if npg > 2049:
            continue  # (the largest size: on the GPU only; its sums obey the same 24-bit argument, asserted below)
        for pad in R.CHAN_PADS:
            x, y, center, scale = R.chan_int_inputs(G, npg, C, pad)
            xr, yr, cr, sr, _ = ZD.chan_inputs(G, npg, C, pad)
            for mode in range(3):
                ref, _ = ZD.chan_ref64(x, y, center, scale, mode, G, npg, C)
                assert R.bits_equal(ZD.chan_emulate32(x, y, center, scale, mode, G, npg, C), ref).all()
                ref, sabs = ZD.chan_ref64(xr, yr, cr, sr, mode, G, npg, C)
                err = np.abs(ZD.chan_emulate32(xr, yr, cr, sr, mode, G, npg, C).astype(F64) - ref)
                assert np.all(err <= (R.K2["chan_reduce"][mode] + npg) * R.U * sabs)
    assert 2 * 80 * max(c[1] for c in R.CHAN_CASES) < 2 ** 24  # |term| <= 80 in halves: every partial sum is a 24-bit number


# ------------------------------------------------------------------------------------------- (1): independent formulations
@pytest.mark.parametrize("kind", range(4))
def test_activation_reference_against_torch(kind):
    f = [lambda v: v, torch.tanh, torch.sigmoid, torch.relu][kind]
    for res in (0, 1):
        case = (kind, res, 257)
        inp = R.make("act_bwd", case)
        x = T(inp["x"]).requires_grad_()
        y = f(x + T(inp["r"]) if res else x)
        close(R.run("act_fwd", case, inp)["y"], y.detach().numpy())
        # the backward is expressed through the output: fed the float64 output, it is autograd's
        y.backward(T(inp["gy"]))
        mine = R.run("act_bwd", case, dict(inp, y=y.detach().numpy()))["gx"]
        sub = np.asarray(inp["x"], F64) + (np.asarray(inp["r"], F64) if res else 0) != 0 if kind == 3 else slice(None)  # (relu'(0))
        close(mine[sub], x.grad.numpy()[sub])


@pytest.mark.parametrize("has_h", (0, 1))
def test_gru_reference_against_autograd(has_h):
    case = (257, has_h)
    inp = R.make("gru_chain", case)
    leaves = {k: T(inp[k]).requires_grad_() for k in ("cu", "cr", "c0") + (("h",) if has_h else ())}
    h = leaves["h"] if has_h else torch.zeros(257, dtype=torch.float64)
    u, r = torch.sigmoid(leaves["cu"]), torch.sigmoid(leaves["cr"])
    co = leaves["c0"] + T(inp["kk"]) * (h * r)
    co.retain_grad()
    o = torch.tanh(co)
    new = h * (1 - u) + o * u
    new.backward(T(inp["g_new"]))
    mine = R.run("gru_chain", case, inp)
    close(mine["hn"], new.detach().numpy())
    close(mine["g_cu"], leaves["cu"].grad.numpy())
    close(mine["g_cr"], leaves["cr"].grad.numpy())
    close(mine["g_co"], co.grad.numpy())
    if has_h:
        close(mine["g_h"], leaves["h"].grad.numpy())
    # the four entry points one by one are the steps of the chain
    a = R.run("gru_gates_fwd", case, inp)
    close(a["u"], u.detach().numpy())
    close(a["hr"], (h * r).detach().numpy())
    b = R.run("gru_out_fwd", case, dict(inp, co=co.detach().numpy(), u=a["u"]))
    close(b["hn"], new.detach().numpy())


@pytest.mark.parametrize("pc", (0, 1))
def test_lstm_reference_against_autograd(pc):
    """submodules.py:357-374: chunks in | remember | out | cell."""
    Ch, npix = 3, 7
    case = (Ch, npix, pc, "none")
    inp = R.make("lstm_bwd", case)
    gates = T(inp["gates"]).requires_grad_()
    prev = T(inp["prev_cell"]).requires_grad_() if pc else None
    i_, r_, o_, c_ = gates.reshape(npix, 4, Ch).unbind(1)
    i_, r_, o_, c_ = torch.sigmoid(i_), torch.sigmoid(r_), torch.sigmoid(o_), torch.tanh(c_)
    cell = (r_ * prev if pc else 0) + i_ * c_
    hidden = o_ * torch.tanh(cell)
    fwd = R.run("lstm_fwd", case, inp)
    close(fwd["cell"], cell.detach().numpy())
    close(fwd["hidden"], hidden.detach().numpy())
    close(fwd["gates"].reshape(npix, 4, Ch)[:, 2], o_.detach().numpy())
    ((hidden * T(inp["g_hidden"])).sum() + (cell * T(inp["g_cell"])).sum()).backward()
    bwd = R.run("lstm_bwd", case, dict(inp, act=fwd["gates"], cell=fwd["cell"]))
    close(bwd["g_gates"], gates.grad.numpy())
    if pc:
        close(bwd["g_prev_cell"], prev.grad.numpy())


@pytest.mark.parametrize("s", range(4))
def test_surrogate_reference_formulas(s):
    """models/spiking_util.py of the reference: arctan 1 / (1 + w x^2), superspike 1 / (1 + w |x|)^2, triangle relu(1 - w |x|),
    multi-Gaussian 1.15 N(0, w) - 0.15 N(w, 6 w) - 0.15 N(-w, 6 w)."""
    case = (s, 1, 257)
    inp = R.make("spike_bwd", case)
    x, w = T(inp["x"]) - T(inp["th"]), float(F32(R.SPIKE_WIDTH[s]))
    n = lambda v, mu, sd: torch.distributions.Normal(mu, sd).log_prob(v).exp()  # noqa: E731
    sg = [1 / (1 + w * x * x), 1 / (1 + w * x.abs()) ** 2, torch.relu(1 - w * x.abs()),
          1.15 * n(x, 0.0, w) - 0.15 * n(x, w, 6 * w) - 0.15 * n(x, -w, 6 * w)][s]
    close(R.run("spike_bwd", case, inp)["gx"], (T(inp["g"]) * sg).numpy(), 1e-7)  # (the kernel's 1 / sqrt(2 pi) is a float32 constant)
    z = R.run("spike_fwd", (0, 1, 257), R.make("spike_fwd", (0, 1, 257)))["z"]
    assert z[0] == 0 and z[1] == 1 and z[2] == 0  # at the threshold, one ulp above, one below


def test_upsampling_references_against_torch():
    for case in R.UP2_CASES:
        if case[4]:
            continue
        inp = R.make("up2_fwd", case)
        x = T(inp["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_()
        y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        close(R.run("up2_fwd", case, inp)["y"], y.detach().permute(0, 2, 3, 1).numpy())
        y.backward(T(inp["gy"]).permute(0, 3, 1, 2))
        close(R.run("up2_bwd", case, inp)["gx"], x.grad.permute(0, 2, 3, 1).numpy())
    for case in R.NEAR_CASES:
        inp = R.make("near_fwd", case)
        x = T(inp["x"])[None].requires_grad_()
        y = F.interpolate(x, scale_factor=case[3], mode="nearest")
        close(R.run("near_fwd", case, inp)["y"], y.detach()[0].numpy())
        y.backward(T(inp["gy"])[None])
        close(R.run("near_bwd", case, inp)["gx"], x.grad[0].numpy())
    for case in R.CUP_CASES:
        chans, B, H, W, pad = case
        inp = R.make("concat_up2", case)
        parts = [torch.zeros(B * H * W, c, dtype=torch.float64) if p is None else T(p)[:, :c] for (c, _), p in zip(chans, inp["parts"])]
        cat = torch.cat(parts, 1).reshape(B, H, W, -1).permute(0, 3, 1, 2)
        y = F.interpolate(cat, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        out = R.run("concat_up2", case, inp)["out"]
        close(out[..., :y.shape[-1]], y)
        assert np.all(out[..., y.shape[-1]:] == R.SENTINEL)


def test_chan_affine_is_the_element_pass_of_batch_norm():
    """The coefficient recipes in the comment above evf_chan_affine, against F.batch_norm in training mode and its autograd."""
    G, npg, C = 1, 257, 3
    case = (G, npg, C, 1)
    inp = R.make("chan_affine", case)
    x = T(inp["x"][:, :C]).requires_grad_()
    g = T(inp["g"][:, :C])
    w, b, eps = T(inp["A"][0]), T(inp["Cc"][0]), 1e-5
    y = F.batch_norm(x, None, None, w, b, training=True, eps=eps)
    mean, var = x.detach().mean(0), x.detach().var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    fwd = R.run("chan_affine", (G, npg, C, 0), dict(inp, g=None, Bc=(w * rstd).numpy()[None], Cc=(b - mean * w * rstd).numpy()[None]))
    close(fwd["out"][:, :C], y.detach().numpy())
    y.backward(g)
    xhat = (x.detach() - mean) * rstd
    S1, S2 = g.sum(0), (g * xhat).sum(0)
    Bc = -(rstd * rstd) * w * S2 / npg
    Cc = -Bc * mean - rstd * w * S1 / npg
    bwd = R.run("chan_affine", case, dict(inp, A=(w * rstd).numpy()[None], Bc=Bc.numpy()[None], Cc=Cc.numpy()[None]))
    close(bwd["out"][:, :C], x.grad.numpy(), 1e-10)


@pytest.mark.parametrize("Cout,n", [(3, 63), (32, 257)])
def test_weight_norm_reference_against_torch(Cout, n):
    case = (Cout, n)
    inp = R.make("wn_bwd", case)
    keep = ~R.wn_overflows(inp["v"])
    v = T(inp["v"]).requires_grad_()
    g = T(inp["g"]).reshape(-1, 1).requires_grad_()
    w = torch._weight_norm(v, g, 0)
    w.backward(T(inp["gw"]))
    fwd = R.run("wn_fwd", case, inp)
    close(fwd["w"], w.detach().numpy())
    close(fwd["nrm"], v.detach().norm(dim=1).numpy())
    bwd = R.run("wn_bwd", case, dict(inp, nrm=fwd["nrm"]))
    close(bwd["gv"][keep], v.grad.numpy()[keep], 1e-9)
    close(bwd["gg"][keep], g.grad.reshape(-1).numpy()[keep], 1e-9)


def test_concat_reference_is_numpy_concatenate():
    for case in R.CASES["concat"]:
        (chans, pad, opad), npix = case
        inp = R.make("concat", case)
        cols = [np.zeros((npix, c)) if p is None else p[:, :c] for (c, _), p in zip(chans, inp["parts"])]
        out = R.run("concat", case, inp)["out"]
        tot = sum(c for c, _ in chans)
        assert np.array_equal(out[:, :tot], np.concatenate(cols, 1)) and np.all(out[:, tot:] == R.SENTINEL)
