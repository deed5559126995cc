"""CPU only: what tests/test_gpu_metrics.py asserts on the device stands on this.  (1) The float64 references of
tests/metrics_ref.py agree with the building blocks of oracle/loss.py run in float64 (fwl's variance, rsat's _avg_ts_term, aee,
masked_window_flow) and with torch's statement of norm_input.  (2) The float32 emulations stay inside the bounds of the GPU test
on its own inputs; the exact cases are exact.  (3) The figures of rule 3 are measured, printed and equal to
metrics_ref.MEASURED.  (4) Every threshold of evf_aee is cleared by 1e-3 relative on every pixel.  (5) Every mutant of
metrics_ref.MUTANTS violates the GPU test's assertion on at least one listed case."""

import types

import numpy as np
import pytest
import torch

import metrics_ref as R
from oracle import loss as OL

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.array(a, F64))  # noqa: E731


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    k = ~np.isnan(b)
    assert np.all(np.abs(a - b)[k] <= tol * (1 + np.abs(b[k]))), float(np.max(np.abs(a - b)[k]))


def results(family, case, dtype=F32, mut=None):
    inp = R.make(family, case)
    exp = R.expect(family, case, inp)
    return exp, R.fractions(exp, Z_outputs(R.run(family, case, inp, dtype, mut)))


def Z_outputs(r):
    return {k: v for k, v in r.items() if not k.startswith("_")}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_stays_inside_the_bounds_of_the_gpu_test(family):
    for case in R.CASES[family]:
        exp, fr = results(family, case)
        for name, f in fr.items():
            assert f <= (0.25 if exp[name].rule == 3 else 1.0), (family, case, name, f)


def test_measured_figures_are_the_stored_ones():
    seen = {}
    for family in R.FAMILIES:
        for case in R.CASES[family]:
            exp, fr = results(family, case)
            for name, f in fr.items():
                if exp[name].rule == 3:
                    seen[exp[name].key] = max(seen.get(exp[name].key, 0.0), f * exp[name].factor())
    print("measured, units of 2^-24 * scale: " + "  ".join(f"{k} {v:.4g}" for k, v in sorted(seen.items())))
    assert set(seen) == set(R.MEASURED)
    for k, v in seen.items():
        assert 0.9 * R.MEASURED[k] <= v <= R.MEASURED[k], (k, v, R.MEASURED[k])


@pytest.mark.parametrize("case", R.AEE_CASES)
def test_aee_thresholds_are_cleared_by_the_margin_on_every_pixel(case):
    inp = R.make("aee", case)
    a, b = R.aee_margins(inp)
    assert a.shape == inp["mask"].shape and np.all(a >= R.AEE_MARGIN) and np.all(b >= R.AEE_MARGIN), (a.min(), b.min())
    err, mag, valid = R.aee_terms(inp, F64)
    gt, m = np.asarray(inp["gt"]), np.asarray(inp["mask"])
    zero = (gt[:, 0] == 0) & (gt[:, 1] == 0)
    # the edges the case must hold: invalid by mask, by gt, by both; one zero component (valid); masks other than 0 and 1; pixels on
    # which exactly one of the two outlier conditions holds, either way round
    assert ((m == 0) & ~zero).any() and ((m != 0) & zero).any() and ((m == 0) & zero).any()
    assert (valid & ((gt[:, 0] == 0) ^ (gt[:, 1] == 0))).any() and (valid & (m != 1)).any()
    assert ((err > 3) & ~(err > 0.05 * mag)).any() and (~(err > 3) & (err > 0.05 * mag)).any()
    # the event counts of avg_ts_ratio are integers: its count is decided exactly
    for tc in R.TS_CASES:
        im = R.make("ts_ratio", tc)["images"]
        assert np.array_equal(im[:, :2], np.round(im[:, :2]))


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_fails_the_gpu_assertion_somewhere(mut):
    failed = [(family, case) for family in R.MUTANT_FAMILIES[mut] for case in R.CASES[family]
              if max(results(family, case, F32, mut)[1].values()) > 1.0]
    print(f"{mut}: fails {len(failed)} cases, the first {failed[:1]}")
    assert failed, mut


def test_exact_cases_are_exact_on_the_reference_alone():
    for family in ("variance", "mask_union", "masked_mean", "pixel_mask"):
        for case in R.CASES[family]:
            if family == "pixel_mask" or case[0] == "exact":
                exp, fr = results(family, case, F64)
                assert all(o.rule == 1 for o in exp.values()) and all(f == 0.0 for f in fr.values()), (family, case)


# ------------------------------------------------------------------------------------------------------ the oracle's blocks
def test_variance_reference_is_the_unbiased_variance_of_fwl():
    for case in R.VAR_CASES:
        inp = R.make("variance", case)
        close(R.run("variance", case, inp)["var"], torch.var(T(inp["img"]), dim=1).numpy(), 1e-9)  # (oracle/loss.py: fwl)


def test_ts_ratio_reference_is_the_oracles_avg_ts_term():
    """_avg_ts_term on one event per (pixel, polarity) that carries the pixel's count as weight and its mean timestamp."""
    for P, HW in R.TS_CASES:
        im = np.asarray(R.make("ts_ratio", (P, HW))["images"], F64)
        lin = torch.arange(HW).repeat(2)[None].repeat(3, 1)
        wgt = T(np.concatenate([im[:, 0], im[:, 1]], 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            ts = T(np.nan_to_num(np.concatenate([im[:, 2] / im[:, 0], im[:, 3] / im[:, 1]], 1), posinf=0.0))
        pol = torch.zeros(3, 2 * HW, 2, dtype=torch.float64)
        pol[:, :HW, 0], pol[:, HW:, 1] = 1.0, 1.0
        # (the timestamp residues at event-free pixels have no event to carry them: left out on both sides)
        ref = OL._avg_ts_term(lin, wgt, ts, pol, (1, HW), float(P))
        mine = R.run("ts_ratio", (P, HW), {"images": np.where(im[:, :2].sum(1, keepdims=True) > 0, im, 0.0) * 1.0})["out"]
        close(mine, ref.numpy(), 1e-6)  # (1e-9 in float64 against the float32 constant)
        assert np.isnan(mine[2]) and bool(torch.isnan(ref[2]))  # no events at all: 0 / 0


@pytest.mark.parametrize("case", R.AEE_CASES)
def test_aee_reference_is_the_oracles(case):
    B, H, W = case
    inp = R.make("aee", case)
    r = R.run("aee", case, inp)
    ratio = np.asarray(inp["ratio"], F64)
    a, p = OL.aee(T(inp["flow"]), T(inp["gt"]), T(inp["mask"]), R.FLOW_SCALING, T(ratio), torch.ones(B, dtype=torch.float64))
    close(r["se"] / (r["nv"] + 1e-9), a.numpy(), 1e-9)
    # the batch-wide outlier sum over the per-sample valid count (the oracle's integer count + 1e-9 is a float32 tensor: 1e-6)
    close(r["no"].sum() / (r["nv"] + 1e-9), p.numpy(), 1e-6)


def test_mask_references_are_the_oracles_masked_window_flow():
    for case in R.MASK_CASES:
        kind, B, P, H, W = case
        inp = R.make("masked_mean", case)
        masks, maps = T(inp["masks"]).reshape(B, P, H, W), T(inp["maps"]).reshape(B, P, 2, H, W)
        win = types.SimpleNamespace(mask=[masks[:, p:p + 1] for p in range(P)], flow_maps=[[maps[:, p]] for p in range(P)])
        ref = OL.masked_window_flow(win, overwrite=False).reshape(B, 2, H * W).numpy()
        close(R.run("masked_mean", case, inp)["out"], ref, 1e-6)
        u = torch.clamp(masks.sum(1), max=1.0).reshape(B, H * W).numpy()  # loss/flow.py:149-150
        close(R.run("mask_union", case, inp)["out"], u)


def test_norm_nonzero_reference_is_norm_input():
    for case in R.NZ_CASES:
        if case[1] > 2000:
            continue
        x = T(R.make("norm_nonzero", case)["x"])
        ref = x.clone()
        nz = ref != 0
        if nz.sum() == 1:
            ref[nz] = float("nan")  # (torch.std of one entry: NaN, with a warning)
        elif nz.any():  # models/model.py:247-252
            ref[nz] = (ref[nz] - ref[nz].mean()) / ref[nz].std()
        close(R.run("norm_nonzero", case, {"x": x.numpy()})["out"], ref.numpy(), 1e-6)  # (mean and std pass through float32)
