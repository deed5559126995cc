"""The evaluation-metric kernels and norm_input through the C ABI, entry point by entry point, against the float64 references of
tests/metrics_ref.py at the bounds stated there and in tests/zoo_ops_ref.py (rule 1: bit for bit; rule 2: an operation count;
rule 3: 4 x a figure measured on the CPU; counts exact), which tests/test_host_metrics_reference.py establishes without a GPU:

evf_image_variance, evf_avg_ts_ratio, evf_aee (and loss.flow.AEE with a batch of three), evf_mask_union, evf_masked_flow_mean,
evf_apply_pixel_mask, evf_norm_nonzero (the default, atomic path) and evf_norm_nonzero_det.

Every float32 buffer handed to a kernel sits between 64 guard elements on either side (tests/gpu_bufs.py), the float64 workspace
of norm_nonzero between guards of its own; outputs are pre-filled with the sentinel; every case ends with the guard check.

EVF_ZOO_OPS_REPORT=<file>: the largest observed error of every output as a fraction of its bound is appended there."""

import numpy as np
import pytest
import torch

import metrics_ref as R
from event_flow_amd import _lib
from gpu_bufs import SENTINEL, Bufs
from test_gpu_zoo_ops import call, out_buf, same_bits, write_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
F32, F64 = np.float32, np.float64

REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    write_report("tests/test_gpu_metrics.py", REPORT)


def judge(family, case, got):
    exp = R.expect(family, case, R.make(family, case))
    for name, f in R.fractions(exp, got).items():
        key = f"{family}.{name} (rule {exp[name].rule})"
        REPORT[key] = max(REPORT.get(key, 0.0), f)
        assert f <= 1.0, f"{family} {case}: {name} at {f:.3g} of its bound (rule {exp[name].rule}): {got[name]} != {exp[name].ref}"


@pytest.mark.parametrize("case", R.VAR_CASES, ids=str)
def test_image_variance(case):
    """exact: integer pixels with an integer mean: the correctly rounded v / (HW - 1).  real: mean 1e3, sigma 1, the two-pass form."""
    kind, Bn, HW = case
    i = R.make("variance", case)
    B = Bufs()
    img, out = B.new(i["img"]), out_buf(B, (Bn,))
    assert call("evf_image_variance", img.ptr, Bn, HW, out.ptr) == 0
    judge("variance", case, {"var": out.get()})
    assert same_bits(img.get(), i["img"])
    B.check()


def test_image_variance_of_one_pixel_is_refused():
    B = Bufs()
    img, out = B.new(np.ones((3, 1), F32)), out_buf(B, (3,))
    assert call("evf_image_variance", img.ptr, 3, 1, out.ptr) == EINVAL
    assert call("evf_image_variance", img.ptr, 0, 2, out.ptr) == EINVAL
    assert (out.get() == SENTINEL).all()
    B.check()


@pytest.mark.parametrize("case", R.TS_CASES, ids=str)
def test_avg_ts_ratio(case):
    """Event-free pixels are out of the count and in the sum of squares; a sample without any event gives what the oracle's rsat
    term gives in float64: 0 / 0 = NaN."""
    P, HW = case
    i = R.make("ts_ratio", case)
    B = Bufs()
    im, out = B.new(i["images"]), out_buf(B, (3,))
    assert call("evf_avg_ts_ratio", im.ptr, 3, HW, float(P), out.ptr) == 0
    got = out.get()
    judge("ts_ratio", case, {"out": got})
    assert np.isnan(got[2]) and not np.isnan(got[:2]).any()
    assert call("evf_avg_ts_ratio", im.ptr, 3, 0, float(P), out.ptr) == EINVAL
    B.check()


@pytest.mark.parametrize("case", R.AEE_CASES, ids=str)
def test_aee_raw_outputs(case):
    """The error sum, the valid count and the outlier count of every sample, each sample with its own ratio; the counts exact."""
    Bn, H, W = case
    i = R.make("aee", case)
    B = Bufs()
    flow, gt, mask, ratio = B.new(i["flow"]), B.new(i["gt"]), B.new(i["mask"]), B.new(i["ratio"])
    out = out_buf(B, (Bn, 3))
    assert call("evf_aee", flow.ptr, gt.ptr, mask.ptr, ratio.ptr, Bn, H, W, R.FLOW_SCALING, out.ptr) == 0
    got = out.get()
    judge("aee", case, {"se": got[:, 0], "nv": got[:, 1], "no": got[:, 2]})
    assert call("evf_aee", flow.ptr, gt.ptr, mask.ptr, None, Bn, H, W, R.FLOW_SCALING, out.ptr) == EINVAL
    B.check()


def test_aee_module_sums_outliers_over_the_batch():
    """loss.flow.AEE with B = 3: the AEE per sample, the outlier percentage = the BATCH-WIDE outlier count over the per-sample
    valid count (loss/flow.py:626 of the reference)."""
    from event_flow_amd.loss import flow as hloss

    case = (3, 33, 70)
    Bn, H, W = case
    i = R.make("aee", case)
    r = R.run("aee", case, i)
    cfg = {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
           "model": {"mask_output": True}}
    m = hloss.AEE(cfg, DEV, flow_scaling=int(R.FLOW_SCALING))
    G = lambda a: torch.from_numpy(np.array(a, F32)).to(DEV)  # noqa: E731
    inputs = {"event_list": torch.zeros(Bn, 4, 4, device=DEV), "event_list_pol_mask": torch.zeros(Bn, 4, 2, device=DEV),
              "event_mask": G(np.asarray(i["mask"]) != 0)[:, None], "gtflow": G(i["gt"]), "dt_input": torch.ones(Bn),
              "dt_gt": torch.from_numpy(np.array(i["ratio"]))}
    m.event_flow_association([G(i["flow"])], inputs)
    a, p = m()
    a, p = a.cpu().double().numpy(), p.cpu().double().numpy()
    exp = R.expect("aee", case, i)["se"]
    assert np.all(np.abs(a - r["se"] / (r["nv"] + 1e-9)) <= (exp.bound() + 2 * R.U * r["se"]) / r["nv"])  # (+ the divide and the 1e-9)
    ref_p = r["no"].sum() / (r["nv"] + 1e-9)
    assert np.all(np.abs(p - ref_p) <= 2 * R.U * ref_p), (p, ref_p)  # exact counts, one float32 sum and one divide
    assert not np.allclose(ref_p, r["no"] / (r["nv"] + 1e-9), rtol=1e-3)  # (the per-sample percentage is something else here)


@pytest.mark.parametrize("case", R.MASK_CASES, ids=str)
def test_mask_union_and_masked_flow_mean(case):
    """Binary masks with dyadic flows: bit for bit; fractional mask weights: rule 2 (union) / rule 3 (mean).  A pixel masked in
    no pass: 0 / 1e-9 = 0."""
    kind, Bn, P, H, W = case
    i = R.make("masked_mean", case)
    B = Bufs()
    masks, maps = B.new(i["masks"]), B.new(i["maps"])
    u, mean = out_buf(B, (Bn, H * W)), out_buf(B, (Bn, 2, H * W))
    assert call("evf_mask_union", masks.ptr, Bn, P, H, W, u.ptr) == 0
    assert call("evf_masked_flow_mean", maps.ptr, masks.ptr, Bn, P, H, W, mean.ptr) == 0
    judge("mask_union", case, {"out": u.get()})
    judge("masked_mean", case, {"out": mean.get()})
    empty = ~np.asarray(i["masks"]).any(1)
    assert empty.any() and not mean.get().transpose(0, 2, 1)[empty].any()
    assert call("evf_mask_union", masks.ptr, Bn, 0, H, W, u.ptr) == EINVAL
    assert call("evf_masked_flow_mean", maps.ptr, None, Bn, P, H, W, mean.ptr) == EINVAL
    assert same_bits(masks.get(), i["masks"]) and same_bits(maps.get(), i["maps"])
    B.check()


@pytest.mark.parametrize("case", R.PIXMASK_CASES, ids=str)
def test_apply_pixel_mask_in_place(case):
    """B * C * HW = 255, 256, 257, ... (both sides of a multiple of the block), C = 1, 2, 5: one multiplication, bit for bit."""
    Bn, C, H, W = case
    i = R.make("pixel_mask", case)
    B = Bufs()
    x, mask = B.new(i["x"]), B.new(i["mask"])
    assert call("evf_apply_pixel_mask", x.ptr, mask.ptr, Bn, C, H, W) == 0
    judge("pixel_mask", case, {"x": x.get()})
    assert same_bits(mask.get(), i["mask"])
    assert call("evf_apply_pixel_mask", x.ptr, mask.ptr, Bn, 0, H, W) == EINVAL
    B.check()


class F64Buf:
    """A float64 workspace between guards of its own, filled with garbage on entry."""

    def __init__(self, n, fill):
        self.full = torch.full((8 + n + 8,), -724625.0, dtype=torch.float64, device=DEV)
        self.t = self.full[8:8 + n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.full[:8] == -724625.0).all() & (self.full[-8:] == -724625.0).all())


@pytest.mark.parametrize("case", R.NZ_CASES, ids=str)
def test_norm_nonzero_both_paths(case):
    """The default (atomic) path from a garbage-filled workspace and the fixed-order twin, which repeats its bits.  n up to
    2^20 + 1: the 1024-block cap and the grid-stride loop.  All zeros stay zeros; exactly one non-zero entry gives NaN there and
    nowhere else, as torch does."""
    kind, n = case
    i = R.make("norm_nonzero", case)
    B = Bufs()
    x = B.new(i["x"])
    out, out_det, out_det2 = out_buf(B, (n,)), out_buf(B, (n,)), out_buf(B, (n,))
    ws = F64Buf(3, 1e30)
    assert call("evf_norm_nonzero", x.ptr, n, out.ptr, ws.t.data_ptr()) == 0
    judge("norm_nonzero", case, {"out": out.get()})
    nws = int(_lib.load().evf_norm_nonzero_det_ws(n))
    assert nws == 3 * min((n + 1023) // 1024, 1024)
    wsd = F64Buf(nws, float("nan"))
    assert call("evf_norm_nonzero_det", x.ptr, n, out_det.ptr, wsd.t.data_ptr(), nws) == 0
    assert call("evf_norm_nonzero_det", x.ptr, n, out_det2.ptr, wsd.t.data_ptr(), nws) == 0
    judge("norm_nonzero", case, {"out": out_det.get()})
    a, b = out_det.get(), out_det2.get()
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the deterministic path does not repeat its bits"
    assert call("evf_norm_nonzero_det", x.ptr, n, out_det.ptr, wsd.t.data_ptr(), nws - 1) == EINVAL
    assert call("evf_norm_nonzero", x.ptr, 0, out.ptr, ws.t.data_ptr()) == EINVAL
    assert same_bits(x.get(), i["x"])
    assert ws.intact() and wsd.intact()
    B.check()
