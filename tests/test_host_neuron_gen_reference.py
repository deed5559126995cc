"""The bounds of the general-path cell kernel tests, established without a GPU: neuron_gen_ref.neuron_ref tied to oracle.snn
(the code the goldens came from), its fp32 emulation in the kernels' operation order measured against it in fp64, and the proof
that the resulting bounds reject eight ways of getting the backward subtly wrong.  tests/test_gpu_neuron_gen.py holds the
kernels to the same bounds."""

import itertools

import numpy as np
import pytest
import torch

import neuron_gen_ref as R
from oracle import snn as osnn

CROSS = [(k, hard, gst, prev) for k in R.KINDS for hard in (True, False) for gst in (True, False) for prev in R.PREV_MODES]


# --------------------------------------------------------------------------------------------- the reference IS the oracle
ORACLE_NAMES = {"lif": ("leak", "thresh"), "plif": ("leak_v", "thresh", "leak_pt", "add_pt"),
                "alif": ("leak_v", "t0", "t1", "leak_t"), "xlif": ("leak_v", "t0", "t1", "leak_pt")}


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_in_fp32_matches_the_oracle_cell(kind):
    """neuron_ref(float32) against oracle.snn.cell_step with a 1x1 identity feed-forward weight (cur = x), forward and every
    gradient, hard / soft reset x the four surrogates.  PLIF / XLIF: the oracle's pooled activity of x with k = 1 is mean_c |x|."""
    B, C, H, W = 2, 12, 3, 5
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()  # noqa: E731
    for hard, surr in itertools.product((True, False), R.SURROGATES):
        width = R.WIDTH[surr]
        x = (2 * rnd(B, C, H, W)).requires_grad_(True)
        v, ax = (2 * rnd(B, C, H, W)).requires_grad_(True), torch.rand(B, C, H, W, generator=gen).requires_grad_(True)
        z = (torch.rand(B, C, H, W, generator=gen) < 0.3).float().requires_grad_(True)
        names = ORACLE_NAMES[kind]
        vals = [rnd(C, 1, 1), torch.tensor([0.005, 0.01, 0.3] * 4).view(C, 1, 1), None, None]
        if kind == "plif":
            vals[2], vals[3] = rnd(C, 1, 1), rnd(C, 1, 1)
        elif kind != "lif":
            vals[2], vals[3] = torch.tensor([-0.1, 0.0, 0.2, 0.2] * 3).view(C, 1, 1), rnd(C, 1, 1)
        p = {"c." + nm: val.clone().requires_grad_(True) for nm, val in zip(names, vals)}
        p["c.ff.weight"] = torch.eye(C).view(C, C, 1, 1)
        p["c.act_width"] = torch.tensor(width)
        state = (v, z) if kind == "lif" else (v, z, ax)
        res = rnd(B, C, H, W).round()
        out, new = osnn.cell_step(kind, p, "c.", x, state, recurrent=False, act=surr, hard_reset=hard, residual=res)
        ups = [rnd(B, C, H, W) for _ in range(4)]
        loss = (ups[0] * new[0]).sum() + (ups[1] * out).sum() + (ups[2] * new[1]).sum()
        if kind != "lif":
            loss = loss + (ups[3] * new[2]).sum()
        wrt = [x, v, z] + ([ax] if kind != "lif" else []) + [p["c." + nm] for nm in names]
        og = torch.autograd.grad(loss, wrt, allow_unused=True)
        # the same through neuron_ref in fp32: the pooled activity is an input there, its gradient g_P flows back into x by hand
        P = x.detach().abs().mean(1).reshape(-1).numpy() if kind in ("plif", "xlif") else None
        up = {"g_v_out": nhwc(ups[0]), "g_z_out": nhwc(ups[1]), "g_z_out2": nhwc(ups[2]),
              "g_aux_out": nhwc(ups[3]) if kind != "lif" else None}
        prm = [None if val is None else val.reshape(-1).numpy() for val in vals]
        r = R.neuron_ref(kind, nhwc(x), nhwc(v), nhwc(z), nhwc(ax) if kind != "lif" else None, P, nhwc(res), prm, hard, surr,
                         width, upstream=up, dtype=torch.float32)
        assert r["v_out"].dtype == np.float32
        tag = f"{kind} hard={hard} {surr}"
        assert np.array_equal(r["out"], nhwc(out)), tag
        np.testing.assert_allclose(r["v_out"], nhwc(new[0]), rtol=1e-6, atol=1e-6, err_msg=tag)
        if kind != "lif":
            np.testing.assert_allclose(r["aux_out"], nhwc(new[2]), rtol=1e-6, atol=1e-6, err_msg=tag)
        g_x = r["g_cur"]
        if P is not None:
            g_x = g_x + np.sign(nhwc(x)) * r["g_P"][:, None] / C
        got = [g_x, r["g_v_prev"]]
        got.append(r["g_z_prev"] if kind == "alif" else np.zeros_like(g_x))  # (z detached in the reset; no recurrent conv)
        if kind != "lif":
            got.append(r["g_aux_prev"])
        got += [r[f"g_p{i}"] for i in range(len(names))]
        for i, (a, b) in enumerate(zip(got, og)):
            b = np.zeros_like(a) if b is None else (nhwc(b) if b.dim() == 4 else b.reshape(-1).numpy())
            np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(b).max())), err_msg=f"{tag} gradient {i}")


# ---------------------------------------------------------------------------------------------------------------- bounds
def _emulation_errors(case, mutant=None):
    """Errors of emulate32 (or a mutant) against the fp64 reference in units of 2^-24 * scale.
    -> {"element": worst per-element output, "sum": worst of parameter sums and g_P, "spikes": mismatches, per output ...}."""
    k, prm, hard = case["kind"], case["params"], case["hard"]
    ins = (case["cur"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], case["residual"])
    fwd = R.emulate32_fwd(k, *ins, prm, hard, mutant=mutant)
    ref = case["ref_fwd"]
    fs = R.forward_scales(k, case["cur"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], prm, hard)
    e = {"spikes": int(np.count_nonzero(fwd["z_out"] != ref["z_out"]) + np.count_nonzero(fwd["out"] != ref["out"]))}
    e["v_out"] = R.units(fwd["v_out"], ref["v_out"], fs["v_out"])
    if k != "lif":
        e["aux_out"] = R.units(fwd["aux_out"], ref["aux_out"], fs["aux_out"])
    bref, sc = R.backward_reference(case, fwd["v_out"], fwd["aux_out"])
    got = R.emulate32_bwd(k, fwd["v_out"], fwd["aux_out"], case["v_prev"], case["z_prev"], case["aux_prev"], case["P"], prm, hard,
                          case["surrogate"], case["width"], case["upstream"], mutant=mutant)
    for nm in R.PER_ELEMENT + R.PARAM_SUMS + ("g_P",):
        if bref[nm] is None:
            continue
        if case["prev"] != "present" and nm in ("g_v_prev", "g_z_prev", "g_aux_prev"):
            continue  # (no previous state, or one that takes no gradient: not written)
        e[nm] = R.units(got[nm], bref[nm], sc[nm])
    e["element"] = max(e[nm] for nm in ("v_out", "aux_out") + R.PER_ELEMENT if nm in e)
    e["sum"] = max(e[nm] for nm in R.PARAM_SUMS + ("g_P",) if nm in e)
    return e


def _case(shape, key):
    k, hard, gst, prev = key
    return R.make_case(k, shape[0], shape[1], hard, gst, prev)


@pytest.fixture(scope="module")
def measured():
    return {(shape, key): _emulation_errors(_case(shape, key)) for shape in R.SMALL_SHAPES for key in CROSS}


def test_bounds_are_four_times_the_emulations_error(measured):
    worst = {q: max(e[q] for e in measured.values()) for q in ("element", "sum")}
    for shape in R.SMALL_SHAPES:
        row = {q: max(e[q] for (s, _), e in measured.items() if s == shape) for q in ("element", "sum")}
        print(f"C {shape[0]:5d} npix {shape[1]:3d}: " + "  ".join(f"{q} {x:.3g}" for q, x in row.items()))
    per_output = {}
    for e in measured.values():
        for nm, x in e.items():
            per_output[nm] = max(per_output.get(nm, 0.0), x)
    print("per output: " + "  ".join(f"{nm} {x:.3g}" for nm, x in per_output.items()))
    print("worst: " + "  ".join(f"{q} {x:.4g}" for q, x in worst.items()))
    print(f"bound: K_E {R.K_E:.4g}  K_SUM {R.K_SUM:.4g}")
    assert all(e["spikes"] == 0 for e in measured.values())  # the margin of the generator holds for the emulation too
    assert R.K_E == 4.0 * R.MEASURED["element"] and R.K_SUM == 4.0 * R.MEASURED["sum"]
    for q, x in worst.items():
        assert x <= R.MEASURED[q], (q, x)
        assert x >= 0.9 * R.MEASURED[q], (q, x)  # ... the recorded figure is the measured one, not a generous guess


def test_chain_term_of_the_launch_geometry():
    """The extra term of the parameter sums follows the launch geometry of evf_neuron_bwd; it stays below 5 + 6 + 4 + 256 (+ 1 for
    the add onto the output) wherever the reductions are the shuffle / in-turns ones."""
    shapes = R.SMALL_SHAPES + R.BLOCK_SHAPES
    for C, npix in shapes:
        g = R.bwd_geometry(C, npix)
        chain, chain_gp = R.chain_terms(C, npix)
        print(f"C {C:5d} npix {npix:6d}: {g}  chain {chain}  g_P {chain_gp}")
        assert g["bs"] % g["Q"] == 0 and g["bs"] <= 256 and g["nblk"] * g["bs"] * g["trips"] >= npix * g["Q"]
        assert g["np2"] == (C in (12, 24, 48, 132, 252, 20, 40))
        if not g["np2"]:
            assert chain <= 5 + 6 + 4 + 256 + 1
        assert chain <= 5 + 85 + 256 + 1  # (not a power of two: up to 255 / 3 threads add into one LDS word)
    # (32, 4097): 64 blocks of three trips with dead lanes in the last one; one block more needs 64 * 1024 float4 + 1
    g = R.bwd_geometry(32, 4097)
    assert g["nblk"] == 64 and g["trips"] == 3 and 4097 * 8 % (64 * 256) != 0
    assert R.bwd_geometry(32, 8200)["nblk"] == 65 and not R.bwd_geometry(32, 8200)["replicas"]
    assert R.bwd_geometry(32, 32768)["nblk"] == 256 and not R.bwd_geometry(32, 32768)["replicas"]
    assert R.bwd_geometry(32, 33000)["replicas"] and R.bwd_geometry(32, 33000)["nblk"] == 258
    g = R.bwd_geometry(32, 140000)
    assert g["nblk"] == 1024 and g["trips"] == 5 and 140000 * 8 > 4096 * 256  # (the forward's 4096-block cap too)
    for C, npix in ((256, 4100), (260, 3100), (384, 2100), (1024, 1100), (24, 45000)):
        assert R.bwd_geometry(C, npix)["replicas"], (C, npix)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    """A kernel that made this mistake would fail the GPU tests: at EVERY small shape the mutant breaks a bound (K_E per element,
    K_SUM + the chain term for the sums, or a spike) in at least one configuration where it applies."""
    for shape in R.SMALL_SHAPES:
        if mutant == "last_pixel_dropped" and shape[1] > 70:
            continue
        chain, chain_gp = R.chain_terms(*shape)
        caught = []
        for key in CROSS:
            if not R.mutant_applies(mutant, *key):
                continue
            e = _emulation_errors(_case(shape, key), mutant)
            over = [nm for nm in ("v_out", "aux_out") + R.PER_ELEMENT if nm in e and e[nm] > R.K_E]
            over += [nm for nm in R.PARAM_SUMS if nm in e and e[nm] > R.K_SUM + chain]
            over += ["g_P"] * int("g_P" in e and e["g_P"] > R.K_SUM + chain_gp) + ["spikes"] * int(e["spikes"] > 0)
            caught += over
        print(f"{mutant} C {shape[0]} npix {shape[1]}: {sorted(set(caught))}")
        assert caught, (mutant, shape)


# ----------------------------------------------------------------------------------------------------- leaky and pretrace
def test_leaky_reference_matches_the_oracle_cell():
    gen = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 8, 3, 4
    for act in R.ACTS:
        x, st, res = (torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) for _ in range(3))
        p = {"c.ff.weight": torch.eye(C, dtype=torch.float64).view(C, C, 1, 1), "c.ff.bias": torch.zeros(C, dtype=torch.float64),
             "c.leak": torch.randn(C, 1, 1, generator=gen, dtype=torch.float64)}
        out, mix = osnn.conv_leaky_step(p, "c.", x, st, act, residual=res)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).numpy()  # noqa: E731
        r = R.leaky_ref(nhwc(x), nhwc(st), nhwc(res), p["c.leak"].reshape(-1).numpy(), act)
        np.testing.assert_allclose(r["mix"], nhwc(mix), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(r["out"], nhwc(out), rtol=1e-13, atol=1e-13)


def test_pretrace_reference_on_a_hand_made_case():
    x = np.zeros((1, 3, 3, 2))
    x[0, 1, 1] = [-2.0, 4.0]  # mean |x| = 3 at the centre
    r = R.pretrace_ref(x, 3, 1, g_P=np.ones((1, 3, 3)))
    np.testing.assert_allclose(r["P"], np.full((1, 3, 3), 3.0 / 9.0))
    # every one of the nine windows covers the centre: g_x = sign(x) / C * 9 / 9; zeros take sign 0
    np.testing.assert_allclose(r["g_x"][0, 1, 1], [-0.5, 0.5])
    assert not r["g_x"][0, 0, 0].any()
    np.testing.assert_allclose(r["s_g_x"][0, 1, 1], [0.5, 0.5])
    np.testing.assert_allclose(r["s_g_x"][0, 0, 0], [4 / 9 / 2, 4 / 9 / 2])  # (a corner lies in four windows)
