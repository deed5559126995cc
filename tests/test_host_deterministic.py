"""Host side of the deterministic contrast-maximisation loss (no GPU): the switch, the C-ABI tables, and the two fixed-point scale
rules of csrc/evf_events.hip (k_cm_splat_det, k_cm_event_sum_det) restated in numpy."""

import os
import subprocess
import sys

import numpy as np

from event_flow_amd import _lib
from event_flow_amd.loss import flow as hloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the switch
def test_environment_sets_the_initial_mode_in_a_fresh_interpreter():
    procs = []
    for env, want in [(None, False), ("0", False), ("1", True)]:  # (three children at once: each pays the import of torch)
        e = {k: v for k, v in os.environ.items() if k != "EVF_DETERMINISTIC"}
        if env is not None:
            e["EVF_DETERMINISTIC"] = env
        procs.append((want, subprocess.Popen([sys.executable, "-c", "from event_flow_amd import _lib; print(int(_lib.deterministic()))"],
                                             cwd=ROOT, env=e, stdout=subprocess.PIPE, text=True)))
    for want, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0 and out.strip() == str(int(want))


def test_setter_getter_and_reexport():
    before = _lib.deterministic()
    try:
        _lib.set_deterministic(True)
        assert _lib.deterministic() is True and hloss.deterministic() is True
        hloss.set_deterministic(0)
        assert _lib.deterministic() is False and hloss.deterministic() is False
    finally:
        _lib.set_deterministic(before)
    assert hloss.set_deterministic is _lib.set_deterministic and hloss.deterministic is _lib.deterministic


def test_the_four_entry_points_are_declared():
    n_fwd, n_bwd = len(_lib.SIGNATURES["evf_cm_loss_fwd"]), len(_lib.SIGNATURES["evf_cm_loss_bwd"])
    assert _lib.SIGNATURES["evf_cm_loss_ws_det"] == _lib.SIGNATURES["evf_cm_loss_ws"]
    assert len(_lib.SIGNATURES["evf_cm_loss_bwd_ws_det"]) == 7
    # the arguments of the default calls, `ws` followed by its size (forward) / `ws` and its size added (backward)
    assert len(_lib.SIGNATURES["evf_cm_loss_fwd_det"]) == n_fwd + 1
    assert len(_lib.SIGNATURES["evf_cm_loss_bwd_det"]) == n_bwd + 2
    assert _lib.RESTYPES["evf_cm_loss_ws_det"] is _lib.L and _lib.RESTYPES["evf_cm_loss_bwd_ws_det"] is _lib.L
    header = open(os.path.join(ROOT, "include", "evflow.h")).read()
    for name in ("evf_cm_loss_ws_det", "evf_cm_loss_fwd_det", "evf_cm_loss_bwd_ws_det", "evf_cm_loss_bwd_det"):
        assert name + "(" in header


# ------------------------------------------------------------------ the scale rules
def fwd_scale_log2(M, P):
    """largest k with M * max(P, 1) * 2^k < 2^62, by search (the module computes it from the bit length)"""
    n, k = M * max(P, 1), 0
    while n * 2 ** (k + 1) < 2 ** 62:
        k += 1
    return k


def fixed_sum(terms, k):
    """the kernels' accumulation: round(term * 2^k) to nearest-even as exact integers, summed, converted once to fp32, * 2^-k"""
    scaled = np.ldexp(terms.astype(np.float64), k)  # (fp32 * 2^k is exact in float64; rint: half to even, as __float2ll_rn)
    assert np.abs(scaled).max() < 2.0 ** 62
    total = int(np.rint(scaled).astype(np.int64).sum(dtype=np.int64))  # (wraps like the hardware would: the caller checks the range)
    return np.ldexp(np.float32(total), -k), total  # np.float32(int): round to nearest


def test_forward_scale_rule():
    assert hloss.cm_det_scale_log2(15000, 10) == 44 and hloss.cm_det_scale_log2(50000, 1) == 46  # c3, c4
    for M, P in [(1, 1), (2, 1), (3, 1), (700, 3), (15000, 10), (50000, 1), (2 ** 20, 1), (2 ** 20 - 1, 7), (2 ** 30 - 1, 1), (2 ** 15, 2 ** 14)]:
        k = hloss.cm_det_scale_log2(M, P)
        assert k == fwd_scale_log2(M, P), (M, P)
        # worst case of the admitted range: every one of the M terms of a pixel at its bound P (|wt * tau * pol| <= P)
        assert M * (P * 2 ** k) < 2 ** 62 and M * max(P, 1) * 2 ** (k + 1) >= 2 ** 62
    assert hloss.cm_det_scale_log2(5, 0) == hloss.cm_det_scale_log2(5, 1)


def test_forward_refusal_boundary():
    assert hloss.CM_DET_MIN_LOG2 == 32
    assert hloss.cm_det_scale_log2(2 ** 30 - 1, 1) == 32 and hloss.cm_det_scale_log2(2 ** 30, 1) == 31
    assert hloss.cm_det_scale_log2(2 ** 20, 2 ** 10 - 1) == 32 and hloss.cm_det_scale_log2(2 ** 20, 2 ** 10) == 31
    assert hloss._det_refusal(2 ** 30 - 1, 1, 64, 64) is None and "2^30" in hloss._det_refusal(2 ** 20, 2 ** 10, 64, 64)
    assert hloss._det_refusal(100, 1, 8, 2048) is None and "2048" in hloss._det_refusal(100, 1, 8, 2049)


def test_backward_exponent_rule():
    for M in (1, 2, 3, 600, 4096, 4097, 15000, 2 ** 29):
        L = int(np.ceil(np.log2(M))) if M > 1 else 0
        for val in (np.float32(1e-45), np.float32(1.1754942e-38), np.float32(1.17549435e-38), np.float32(3e-7), np.float32(1.0),
                    np.float32(1.9999999), np.float32(2.0), np.float32(123456.7), np.finfo(np.float32).max):
            bits = int(np.float32(val).view(np.uint32))
            e = hloss.cm_det_grad_exp(bits, M)
            E = max((bits >> 23) & 0xFF, 1)
            assert e == 187 - L - E
            worst = int(np.rint(np.ldexp(np.float64(val), e)))  # every one of the M terms of a pixel as large as the maximum
            assert M * worst < 2 ** 62, (M, val)
            assert 2 ** L * 2 ** (E - 126 + e) == 2 ** 61  # the bound the rule is built on, met with equality


def test_fixed_point_sum_is_order_independent_and_no_worse_than_fp32():
    rng = np.random.default_rng(2024)
    n = 10 ** 4
    # forward rule: terms in [-1, 1] (P = 1); backward rule: terms of any magnitude, scaled by their maximum
    fwd = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    bwd = (rng.standard_normal(n) * np.exp(rng.uniform(-12, 3, n))).astype(np.float32)
    kf = hloss.cm_det_scale_log2(n, 1)
    kb = hloss.cm_det_grad_exp(int(np.abs(bwd).max().view(np.uint32)), n)
    for terms, k in ((fwd, kf), (bwd, kb)):
        ref, itot = fixed_sum(terms, k)
        assert abs(itot) < 2 ** 62
        for _ in range(16):
            got, _ = fixed_sum(terms[rng.permutation(n)], k)
            assert got == ref and got.dtype == np.float32
        exact = float(np.sum(terms.astype(np.float64)))
        seq = np.cumsum(terms, dtype=np.float32)[-1]  # (cumsum adds one term after the other in fp32)
        assert abs(float(ref) - exact) <= abs(float(seq) - exact), (float(ref), float(seq), exact)
