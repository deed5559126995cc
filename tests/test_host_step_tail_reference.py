"""The bounds of the clip + Adam tests, established without a GPU: the fp32 emulation of the kernels (step_tail_ref.adam_ref with
dtype=float32) against the fp64 reference, and the proof that those bounds are tight enough to reject every listed way of
getting the optimizer subtly wrong.  tests/test_gpu_step_tail.py holds the kernels to the same bounds."""

import numpy as np
import pytest

import step_tail_ref as R

SIZES = (5, 1025, 75011)


@pytest.fixture(scope="module")
def measured():
    """Worst normalised error of the emulation per (size, regime), computed once."""
    return {(n, rg): R.run_emulation(n, rg) for n in SIZES for rg in R.REGIMES}


def test_bounds_are_four_times_the_emulations_error(measured):
    worst = {k: max(e[k] for e in measured.values()) for k in ("p", "m", "v", "sumsq")}
    for (n, rg), e in measured.items():
        print(f"n {n:6d} {rg:8s}: " + "  ".join(f"{k} {x:.3g}" for k, x in e.items()))
    print("worst: " + "  ".join(f"{k} {x:.4g}" for k, x in worst.items()))
    print("bound: " + "  ".join(f"{k} {x:.4g}" for k, x in R.BOUND.items()))
    for k, x in worst.items():
        assert R.BOUND[k] == 4.0 * R.MEASURED[k]
        assert x <= R.BOUND[k] / 4.0, (k, x)
        # ... and the recorded figure is the measured one, not a generous guess
        assert x >= 0.9 * R.MEASURED[k], (k, x)


def test_inputs_cover_what_the_bounds_are_for():
    p, s = R.make_inputs(75011)
    assert np.count_nonzero(p == 0) > 1000 and np.abs(p[p != 0]).min() < 2e-6 and np.abs(p).max() > 0.5
    for rg in R.REGIMES:
        _, max_norm, gs = R.case_inputs(75011, rg)
        g = gs[0].astype(np.float64)
        norm = np.sqrt(np.sum(g * g))
        assert np.count_nonzero(np.abs(g) < 1e-9) > 1000  # eps = 1e-8 dominates sqrt(v_hat) there
        if rg == "above":
            assert max_norm > 10 * norm
        if rg == "clipped":
            assert 0.5e-3 < norm < 2e-3 and abs(max_norm * 10 - 1e-3) < 1e-9
            assert np.abs(g).min() ** 2 * 0.01 * 1e-3 > 1.2e-38  # (1 - b2) (g coef)^2 is a normal fp32 number


def test_fp64_reference_matches_torch_adam():
    """adam_ref(float64) IS clip_grad_norm_ + torch.optim.Adam (with the ABI's fp32-rounded hyper-parameters)."""
    import torch

    f = lambda x: float(np.float32(x))  # noqa: E731
    for rg in R.REGIMES:
        p0, max_norm, gs = R.case_inputs(1025, rg)
        w = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
        opt = torch.optim.Adam([w], lr=f(R.LR), betas=(f(R.B1), f(R.B2)), eps=f(R.EPS))
        p, m, v = p0.astype(np.float64), np.zeros(1025), np.zeros(1025)
        for t, g in enumerate(gs[:4], 1):
            w.grad = torch.from_numpy(g.astype(np.float64))
            if max_norm > 0:
                torch.nn.utils.clip_grad_norm_([w], f(max_norm))
            opt.step()
            p, m, v, _ = R.adam_ref(p, g, m, v, max_norm=max_norm, t=t, dtype=np.float64)
            np.testing.assert_allclose(w.detach().numpy(), p, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(opt.state[w]["exp_avg"].numpy(), m, rtol=1e-12, atol=0)
            np.testing.assert_allclose(opt.state[w]["exp_avg_sq"].numpy(), v, rtol=1e-12, atol=0)


@pytest.mark.parametrize("mutation", R.MUTANTS)
def test_every_mutant_exceeds_the_bounds(mutation):
    """A kernel that made this mistake would fail the GPU tests: at EVERY size the mutant breaks a bound in at least one
    clip regime."""
    for n in SIZES:
        caught = []
        for rg in R.REGIMES:
            e = R.run_emulation(n, rg, mutation)
            over = [k for k in e if e[k] > R.BOUND[k]]
            print(f"{mutation} n {n:6d} {rg:8s}: " + "  ".join(f"{k} {x:.3g}" for k, x in e.items()) + f"  -> {over}")
            caught += over
        assert caught, (mutation, n)


def test_finalize_ref_on_a_hand_made_case():
    """The collection reference against numbers worked out by hand."""
    slab = np.zeros((2, R.NW))
    slab[0, (4 * 32 + 3) * 32 + 7] = 5.0  # tap 4 (centre), ci 3, co 7
    slab[1, (4 * 32 + 3) * 32 + 7] = 2.0
    slab[1, (8 * 32 + 0) * 32 + 31] = -1.0  # tap 8 (dy 2, dx 2), ci 0, co 31
    dst = np.ones((32, 32, 3, 3))
    small = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    rows = np.arange(18.0).reshape(3, 6)  # column sums 18 21 24 27 30 33
    head = np.array([[10.0, 20.0], [1.0, 2.0]])  # columns 4, 5 (head_off 4)
    out = R.finalize_ref([slab], [dst], small, 1, rows, head, 4, [np.array([100.0, 100.0]), np.array([0.0, 0.0, 0.0])],
                         [0, 3], [2, 3], [2, 0])
    assert out["slab_dst"][0][7, 3, 1, 1] == 8.0 and out["slab_dst"][0][31, 0, 2, 2] == 0.0 and out["slab_dst"][0].sum() == NW_ONES + 6.0
    np.testing.assert_array_equal(out["seg_dst"][0], [100 + 1 + 18, 100 + 2 + 21])
    np.testing.assert_array_equal(out["seg_dst"][1], [4 + 27, 5 + 30 + 11, 6 + 33 + 22])
    np.testing.assert_array_equal(out["small"], [0, 0, 3, 0, 0, 0])
    # segment 0 (seg_rows 2): columns 0, 1 of rows 0, 1; segment 1 (all rows): columns 3 .. 5; column 2 belongs to no segment
    np.testing.assert_array_equal(out["rows"], [[0, 0, 2, 0, 0, 0], [0, 0, 8, 0, 0, 0], [12, 13, 14, 0, 0, 0]])
    np.testing.assert_array_equal(out["head_rows"], head)


NW_ONES = float(R.NW)
