"""The bounds of tests/conv_ref.py, established on the CPU: the split emulation is exact, K_IMP and K_SUM follow from emulating the
kernels' arithmetic with a 2x margin, and the bounds reject the wrong kernels they are there for -- each droppable term of the
six-term product removed, x rounded to bf16 before the product (a missed redo flag of the weight gradient), a wrong tap at an image
border, a missing last channel of a ragged group.  The case builders of the impulse leg are checked against the dense float64
references, so the GPU module's expectations are not circular.  No GPU."""

import math

import numpy as np
import pytest

import conv_ref as R

F32, F64 = np.float32, np.float64
N_PROD = 200000


@pytest.fixture(scope="module")
def products():
    rng = np.random.default_rng(20250101)
    return {"full": R.full_values(rng, N_PROD), "exact": R.exact_values(rng, N_PROD), "w": R.weights(rng, N_PROD)}


def test_three_way_split_is_exact_and_every_plane_is_a_bf16(products):
    for v in (products["full"], products["w"], products["exact"]):
        hi, mid, lo = R.split3(v)
        assert np.array_equal(hi.astype(F64) + mid.astype(F64) + lo.astype(F64), v.astype(F64))
        for p in (hi, mid, lo):
            assert R.is_bf16(p).all()
    _, mid, lo = R.split3(products["full"])
    assert (mid != 0).all() and (lo != 0).all()  # full values exercise all six terms
    _, mid, lo = R.split3(products["exact"])
    assert not mid.any() and not lo.any()


def test_k_imp_is_twice_the_emulated_error_and_at_most_16(products):
    x, xe, w = products["full"], products["exact"], products["w"]
    worst = {}
    for rev in (False, True):
        worst["six", rev] = R.units(R.split_product(x, w, reverse=rev), x, w).max()
        worst["six on exact x", rev] = R.units(R.split_product(xe, w, reverse=rev), xe, w).max()
        worst["three", rev] = R.units(R.split_product(xe, w, R.TERMS3, reverse=rev), xe, w).max()
    for k, v in worst.items():
        print(f"  {k}: {v:.3f} units of 2^-24 |x w|")
    k_imp = math.ceil(2 * max(worst.values()))
    print(f"  K_IMP from the emulation: {k_imp}")
    assert k_imp <= R.K_IMP <= k_imp + 1  # (the constant, not a number that moves with the sample)
    assert R.K_IMP <= R.K_IMP_MAX == 16
    # the vote is an optimisation: six terms on an exact x are the three terms plus exact zeros
    assert np.array_equal(R.split_product(xe, w), R.split_product(xe, w, R.TERMS3))
    # the fp32 kernels: one correctly rounded product
    assert R.units(R.f32_product(x, w), x, w).max() <= R.K_F32


@pytest.mark.parametrize("k_bound", [R.K_IMP, R.K_IMP_MAX])
def test_every_dropped_term_violates_the_impulse_bound_on_most_products(products, k_bound):
    x, w = products["full"], products["w"]
    for name, term in R.DROPPABLE.items():
        for rev in (False, True):
            share = float((R.units(R.split_product(x, w, drop=term, reverse=rev), x, w) > k_bound).mean())
            print(f"  K {k_bound} without {name} (reversed {rev}): {100 * share:.1f} % of the full-valued products violate")
            assert share > 0.5, (name, share)
            if name in ("x0w1", "x1w0"):  # second order: 2^-8 of the product
                assert share > 0.99, (name, share)


def test_x_rounded_to_bf16_violates_the_impulse_bound_everywhere(products):
    x, w = products["full"], products["w"]
    share = float((R.units(R.split_product(R.bf16_rne(x), w), x, w) > R.K_IMP_MAX).mean())
    assert share > 0.99, share
    share = float((R.units(R.f32_product(R.bf16_rne(x), w), x, w) > R.K_IMP_MAX).mean())
    assert share > 0.99, share


IMPULSE_SHAPES = [(1, 4, 8, 9, 7, 3, 1), (2, 66, 16, 10, 13, 3, 1), (3, 5, 7, 11, 13, 3, 2), (1, 20, 36, 10, 13, 3, 2), (1, 6, 8, 13, 10, 5, 1),
                  (1, 16, 16, 15, 15, 7, 2), (1, 32, 3, 17, 33, 1, 1), (3, 64, 40, 4, 7, 3, 1)]


@pytest.mark.parametrize("shape", IMPULSE_SHAPES)
def test_impulse_cases_agree_with_the_dense_references(shape):
    """Every output of an impulse case is one product or nothing, the expectation equals the dense float64 convolution of the same
    operands bit for bit, both lattice phases reach both borders, and the rounds put an impulse into every contraction channel."""
    B, Cin, Cout, H, W, k, s = shape
    w = R.weights(np.random.default_rng(3), (Cout, Cin, k, k))
    for direction in ("fwd", "dgrad"):
        K = Cin if direction == "fwd" else Cout
        seen = np.zeros(K, bool)
        kinds = set()
        rounds = R.impulse_rounds(shape, direction)
        for phase in (0, 1):
            for rnd in range(rounds):
                c = R.impulse_case(shape, direction, phase, rnd, w)
                dense = R.conv_fwd64(c["src"], w, s) if direction == "fwd" else R.conv_dgrad64(c["src"], w, s, H, W)
                assert np.array_equal(dense, c["ref"]) and np.array_equal(c["hit"], c["ref"] != 0)
                assert np.count_nonzero(c["src"]) == c["nsites"]
                src = c["src"]
                assert src[:, 0 if phase == 0 else -1].any() and src[:, :, 0 if phase == 0 else -1].any()  # the anchored border
                seen |= src.any((0, 1, 2))
                full = ~R.is_bf16(c["val"])
                for g in range((K + 15) // 16):
                    m = c["chan"] // 16 == g
                    if m.any():
                        kinds.add("full" if full[m].all() else ("exact" if not full[m].any() else "mixed"))
        assert seen.all(), (direction, np.flatnonzero(~seen))
        assert "mixed" in kinds and (K < 16 or len(kinds) >= 2), kinds
        if K >= 48:  # three or more 16-channel groups: the votes see all-exact, all-full and mixed groups
            assert kinds == {"exact", "full", "mixed"}, kinds


def test_promise_cases_hold_full_values_only_below_exact_from():
    shape = (2, 132, 32, 16, 34, 3, 1)
    w = R.weights(np.random.default_rng(4), (32, 132, 3, 3))
    for ef in (0, 4):
        full_seen = False
        for phase in (0, 1):
            c = R.impulse_case(shape, "fwd", phase, 0, w, exact_from=ef)
            assert R.is_bf16(c["src"][..., ef:]).all()
            full_seen |= bool((~R.is_bf16(c["src"][..., :ef])).any()) if ef else False
        assert full_seen == (ef > 0)


@pytest.mark.parametrize("shape,nsplit", [((2, 36, 32, 17, 23, 3, 1), 8), ((2, 72, 100, 17, 23, 3, 1), 4), ((2, 132, 32, 17, 23, 3, 1), 8), ((2, 32, 64, 12, 12, 3, 2), 3),
                                          ((1, 32, 5, 17, 33, 1, 1), 1), ((2, 6, 8, 12, 10, 5, 1), 1), ((1, 16, 16, 14, 14, 7, 2), 1)])
def test_wgrad_impulse_cases_and_the_missed_redo_flag(shape, nsplit):
    """One impulse per input channel: the expectation equals the dense float64 weight gradient; the redo tiles (32 * CT channels) are
    all exact or hold exactly one full value; the impulses use corners / edges AND split boundaries in raster and in tile order;
    and a weight gradient that rounds that one value to bf16 (a missed redo flag of its tile) violates the impulse bound on more
    than 99 % of the elements that value reaches."""
    B, Cin, Cout, H, W, k, s = shape
    c = R.wgrad_case(shape, nsplit)
    assert np.array_equal(R.conv_wgrad64(c["x"], c["gy"], k, s), c["ref"])
    assert (np.count_nonzero(c["x"], axis=(0, 1, 2)) == 1).all()
    per_tile = np.bincount(c["tile"], weights=c["full"])
    assert set(per_tile) <= {0.0, 1.0} and per_tile.max() == 1 and np.array_equal(~R.is_bf16(c["val"]), c["full"])
    if Cin > 64:
        assert per_tile.min() == 0  # an all-exact tile beside a flagged one
    groups = R.wgrad_site_groups(B, H, W, nsplit, s)
    used = set(c["sites"])
    assert all(used & set(g) for g in groups), [len(used & set(g)) for g in groups]
    assert not c["hit"].all() or k == 1  # corners and edges: some taps fall outside the image
    rounded = R.conv_wgrad64(R.bf16_rne(c["x"]), c["gy"], k, s)
    reached = c["hit"] & c["full"][None, :, None, None]
    bad = np.abs(rounded - c["ref"]) > R.K_IMP_MAX * R.U * np.abs(c["ref"])
    assert reached.any() and bad[reached].mean() > 0.99 and not bad[~reached].any()
    e = R.wgrad_case(shape, nsplit, kinds="exact")
    assert R.is_bf16(e["x"]).all()


def test_wgrad_sites_cover_corners_edges_and_split_boundaries():
    B, H, W, ns = 2, 17, 23, 8
    pts = R.wgrad_sites(B, H, W, ns)
    assert len(set(pts)) == len(pts) and set(pts) == set().union(*R.wgrad_site_groups(B, H, W, ns))
    for b in (0, B - 1):
        assert {(b, 0, 0), (b, 0, W - 1), (b, H - 1, 0), (b, H - 1, W - 1), (b, 0, W // 2), (b, H // 2, 0)} <= set(pts)
    flat = {(b * H + y) * W + x for b, y, x in pts}
    npix = B * H * W
    for z in range(ns):
        assert (z * npix) // ns in flat and ((z + 1) * npix) // ns - 1 in flat


DENSE_SHAPES = [((2, 66, 16, 10, 13, 3, 1), 1), ((1, 20, 96, 18, 34, 3, 1), 3), ((1, 132, 30, 17, 33, 3, 1), 3), ((2, 6, 8, 12, 10, 5, 1), 1),
                ((1, 64, 32, 12, 12, 3, 2), 2)]


@pytest.fixture(scope="module")
def dense_cases():
    out = []
    for shape, nslab in DENSE_SHAPES:
        B, Cin, Cout, H, W, k, s = shape
        rng = np.random.default_rng(Cin)
        for kind in ("real", "spikes", "mixed"):
            x, w = R.dense_inputs(rng, (B, H, W, Cin), kind), R.weights(rng, (Cout, Cin, k, k))
            out.append((shape, nslab, kind, x, w, R.conv_fwd64(x, w, s), R.conv_fwd64(np.abs(x), np.abs(w), s)))
    return out


def test_k_sum_is_twice_the_emulated_error_of_the_kernels_association(dense_cases):
    worst = 0.0
    for shape, nslab, kind, x, w, ref, scale in dense_cases:
        u = float(R.dense_units(R.emulate_dense_fwd(x, w, shape[6], nslab), ref, scale).max())
        print(f"  {shape} {kind} {nslab} slab(s): {u:.3f} units of 2^-24 A_e")
        worst = max(worst, u)
    k_sum = math.ceil(2 * worst)
    print(f"  K_SUM from the emulation: {k_sum}")
    assert k_sum <= R.K_SUM <= k_sum + 1


@pytest.mark.parametrize("mutant", ["border", "tail"])
def test_dense_bound_rejects_a_wrong_border_tap_and_a_missing_tail_channel(dense_cases, mutant):
    for shape, nslab, kind, x, w, ref, scale in dense_cases:
        u = R.dense_units(R.emulate_dense_fwd(x, w, shape[6], nslab, mutate=mutant), ref, scale)
        bad = u > R.K_SUM
        assert bad.any(), (shape, kind)
        if mutant == "border":  # only border outputs read the padding
            assert not bad[:, 1:-1, 1:-1].any() or shape[5] > 3 or shape[6] > 1
        else:  # the last channel reaches every output
            assert bad.mean() > 0.5, (shape, kind, bad.mean())


def test_dense_references_are_transposes_of_each_other():
    """<conv(x), g> = <x, conv^T(g)> = <w, wgrad(x, g)> in float64, for both strides and an even-sized image."""
    rng = np.random.default_rng(9)
    for B, Cin, Cout, H, W, k, s in ((2, 5, 7, 11, 13, 3, 2), (1, 6, 4, 12, 10, 5, 1), (1, 3, 4, 8, 8, 3, 2), (1, 4, 3, 6, 7, 1, 1)):
        x, w = rng.standard_normal((B, H, W, Cin)), rng.standard_normal((Cout, Cin, k, k))
        y = R.conv_fwd64(x, w, s)
        g = rng.standard_normal(y.shape)
        a, b, c = (y * g).sum(), (x * R.conv_dgrad64(g, w, s, H, W)).sum(), (w * R.conv_wgrad64(x, g, k, s)).sum()
        assert abs(a - b) <= 1e-10 * abs(a) and abs(a - c) <= 1e-10 * abs(a)
