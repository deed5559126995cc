"""The deterministic voxel binning and IWE splats on the GPU (evf_encode_events_det / evf_encode_window_det / evf_iwe_splat_det
behind loss.flow.set_deterministic): order independence bit for bit, parity with the goldens at the project's bars, with the default
path and with a float64 evaluation, known answers that are exact in fp32, the refusals, and which entry points run."""

import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

from event_flow_amd import _lib, synthetic  # noqa: E402
from event_flow_amd.dataloader import encodings as enc  # noqa: E402
from event_flow_amd.loss import flow as hloss  # noqa: E402
from event_flow_amd.utils import iwe as hiwe  # noqa: E402
from oracle import encodings as oenc  # noqa: E402
from oracle import iwe as oiwe  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVF_OK, EVF_EINVAL, EVF_ENOTSUP = 0, -22, -95
P3 = 3  # passes of every window below
NAMES6 = ["evf_encode_events", "evf_encode_window", "evf_iwe_splat", "evf_encode_events_det", "evf_encode_window_det",
          "evf_iwe_splat_det"]


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def cfg(H, W, overwrite=False):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": overwrite},
            "model": {"mask_output": True}}


class mode:
    """the switch inside a with-block, restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = _lib.deterministic()
        _lib.set_deterministic(self.on)

    def __exit__(self, *exc):
        _lib.set_deterministic(self.before)


@pytest.fixture
def det_on():
    with mode(True):
        yield


# ------------------------------------------------------------------ shapes
# (B, H, W, events per pass), then what is special.  Rows of a stripe: 16384 / (planes * W) capped at H, halved while above 8 (fewer
# than 512 blocks at these sizes).
GEOMETRY = {
    "stripes": ((2, 24, 40, 700), {}),                  # rows 6: several full stripes
    "ragged": ((3, 37, 53, 900), {}),                   # rows 4: short last stripe, ragged width
    "widest": ((1, 3, 2048, 600), {}),                  # nch = 4: rows 2, nb = 5: rows 1 -- the smallest stripe the rule gives
    "crowded": ((2, 70, 41, 2000), {"crowd": True}),    # all events in rows H-6 .. H-2: many terms in each slot
    "leaving": ((2, 24, 40, 600), {"amp": 1.0}),        # flows large enough that events warp outside the image
}


def make_window(name, empty=None):
    """P3 passes of events [B,n,4] (t,y,x,p), their polarity masks and a flow map [B,2,H,W] per pass"""
    (B, H, W, n), opt = GEOMETRY[name]
    rng = np.random.default_rng(5)
    amp = opt.get("amp", 0.1)
    win = dict(B=B, H=H, W=W, n=n, ev=[], pol=[], flows=[])
    for k in range(P3):
        ev = synthetic.event_list_batch(B, n, H, W, 300 + k)
        if opt.get("crowd"):
            ev[:, :, 1] = np.floor(ev[:, :, 1] / H * 5.0) + (H - 6)
        if empty == k:
            ev[:, :, 3] = 0.0  # padding only
        win["ev"].append(ev)
        win["pol"].append(np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], 2).astype(np.float32))
        win["flows"].append(rng.uniform(-amp, amp, size=(B, 2, H, W)).astype(np.float32))
    return win


def permuted(win, seed=77):
    """the same SET of events: those of each pass of each sample in another order, polarity masks alike -> (window, permutations)"""
    rng = np.random.default_rng(seed)
    out, perms = dict(win, ev=[], pol=[]), []
    for ev, pol in zip(win["ev"], win["pol"]):
        ev2, pol2, pp = ev.copy(), pol.copy(), []
        for b in range(ev.shape[0]):
            p = rng.permutation(ev.shape[1])
            ev2[b], pol2[b] = ev[b, p], pol[b, p]
            pp.append(p)
        out["ev"].append(ev2)
        out["pol"].append(pol2)
        perms.append(pp)
    return out, perms


_WIN = {}


def window(name):
    """every window and its permutation once, shared by the cases below, never modified"""
    if name not in _WIN:
        win = make_window(name)
        _WIN[name] = (win,) + permuted(win)
    return _WIN[name]


# ------------------------------------------------------------------ the calls under test
def voxels(win, nb, round_ts):
    """the three binning calls in the mode in force -> dict of arrays"""
    B, H, W = win["B"], win["H"], win["W"]
    ev0 = win["ev"][0]
    out = {}
    e = G(ev0[0])
    out["to_voxel"] = N(enc.events_to_voxel(e[:, 2], e[:, 1], e[:, 0], e[:, 3], nb, sensor_size=(H, W), round_ts=round_ts))
    d = enc.encode_event_list(G(ev0), nb, (H, W), round_ts=round_ts)
    out["list"] = {k: N(v) for k, v in d.items() if k != "event_list"}
    many = enc.encode_window(G(np.stack(win["ev"], 1)), nb, (H, W), round_ts=round_ts)
    assert len(many) == P3
    out["window"] = [{k: N(v) for k, v in d.items() if k != "event_list"} for d in many]
    torch.cuda.synchronize()
    return out


def metrics(win, overwrite):
    """a three-pass record through the validation metrics in the mode in force -> dict of arrays"""
    B, H, W = win["B"], win["H"], win["W"]
    c = cfg(H, W, overwrite)
    S = float(max(H, W))
    fwl, rsat = hloss.FWL(c, DEV, flow_scaling=S), hloss.RSAT(c, DEV, flow_scaling=S)
    last = None
    for k in range(P3):
        last = G(win["flows"][k])
        inputs = {"event_list": G(win["ev"][k]), "event_list_pol_mask": G(win["pol"][k]), "event_mask": torch.ones(B, 1, H, W, device=DEV),
                  "dt_input": torch.tensor([1.0]), "dt_gt": torch.tensor([1.0])}
        for m in (fwl, rsat):
            m.event_flow_association([last], inputs)
    if overwrite:
        for m in (fwl, rsat):
            m.overwrite_intermediate_flow([last])
    out = {"fwl": N(fwl()), "rsat": N(rsat()),
           "ts_images": N(rsat._splat(round_idx=True, nch=4, with_ts=True)),            # what RSAT divides
           "ts_images_bilinear": N(rsat._splat(round_idx=False, nch=4, with_ts=True)),
           "window_iwe_bilinear": N(fwl.compute_window_iwe(round_idx=False)),
           "window_iwe": N(fwl.compute_window_iwe()),
           "window_events": N(fwl.compute_window_events())}
    torch.cuda.synchronize()
    return out


def pol_iwes(win, round_idx):
    """compute_pol_iwe and deblur_events of pass 0 in the mode in force"""
    H, W = win["H"], win["W"]
    ev, pol, fl = G(win["ev"][0]), G(win["pol"][0]), G(win["flows"][0])
    S = float(max(H, W))
    out = {"pol_iwe": N(hiwe.compute_pol_iwe(fl, ev, (H, W), pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=S, round_idx=round_idx)),
           "deblur": N(hiwe.deblur_events(fl, ev, (H, W), flow_scaling=S, round_idx=round_idx)),
           "deblur_pos": N(hiwe.deblur_events(fl, ev, (H, W), flow_scaling=S, round_idx=round_idx, polarity_mask=pol[:, :, 0:1]))}
    torch.cuda.synchronize()
    return out


_RES = {}


def results(kind, name, on, *args):
    """voxels / metrics / pol_iwes of the un-permuted window once per mode; shared, never modified"""
    key = (kind, name, on) + args
    if key not in _RES:
        with mode(on):
            _RES[key] = {"voxels": voxels, "metrics": metrics, "pol_iwes": pol_iwes}[kind](window(name)[0], *args)
    return _RES[key]


# ------------------------------------------------------------------ float64 evaluations (the oracle's formulas, in float64)
def voxel_f64(ev, nb, H, W, round_ts):
    """ev [B,n,4] -> [B,nb,H,W] float64 (oracle/encodings.py:43-55)"""
    ev = ev.astype(np.float64)
    out = np.zeros((ev.shape[0], nb, H * W))
    for b in range(ev.shape[0]):
        t, y, x, p = ev[b].T
        keep = (p != 0) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        t = t * (nb - 1)
        if round_ts:
            t = np.rint(t)
        px = (y.astype(np.int64) * W + x.astype(np.int64))[keep]
        for k in range(nb):
            np.add.at(out[b, k], px, (p * np.maximum(0.0, 1.0 - np.abs(t - k)))[keep])
    return out.reshape(ev.shape[0], nb, H, W)


def iwe_f64(flow, ev, H, W, S, tref, w0, w1, nch, round_idx):
    """flow [B,2,H,W], ev [B,M,4], weights [B,M] -> [B,nch,H,W] float64: (I_w0, I_w1, TS_w0, TS_w1) (oracle/iwe.py:13-95)"""
    B, M, _ = ev.shape
    ev, flow = ev.astype(np.float64), flow.astype(np.float64).reshape(B, 2, H * W)
    out = np.zeros((B, nch, H * W))
    for b in range(B):
        t, y, x = ev[b, :, 0], ev[b, :, 1], ev[b, :, 2]
        lin = (y * W + x).astype(np.int64)
        wy = y + (tref - t) * flow[b, 1, lin] * S
        wx = x + (tref - t) * flow[b, 0, lin] * S
        if round_idx:
            taps = [(np.rint(wy), np.rint(wx), np.ones(M))]
        else:
            taps = []
            for cy in (np.floor(wy), np.floor(wy + 1.0)):
                for cx in (np.floor(wx), np.floor(wx + 1.0)):
                    taps.append((cy, cx, np.maximum(0.0, 1.0 - np.abs(wy - cy)) * np.maximum(0.0, 1.0 - np.abs(wx - cx))))
        a = [np.ones(M) if w0 is None else w0[b].astype(np.float64), np.zeros(M) if w1 is None else w1[b].astype(np.float64)]
        for cy, cx, wt in taps:
            ok = (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            px = (cy[ok] * W + cx[ok]).astype(np.int64)
            for c in range(nch):
                np.add.at(out[b, c], px, (wt * a[c & 1] * (t if c >= 2 else 1.0))[ok])
    return out.reshape(B, nch, H, W)


# ------------------------------------------------------------------ 1: order independence, voxel
@pytest.mark.parametrize("round_ts", [False, True])
@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_1_voxel_grids_do_not_depend_on_the_order_of_the_events(name, nb, round_ts, det_on):
    """The same SET of events in another order within every pass of every sample gives the same voxel bits from all three binning
    calls; cnt / mask / pol (un-permuted back) are the default entry point's bits."""
    win, other, perms = window(name)
    assert all(not np.array_equal(a, b) for a, b in zip(win["ev"], other["ev"]))
    a = results("voxels", name, True, nb, round_ts)
    b = voxels(other, nb, round_ts)
    plain = results("voxels", name, False, nb, round_ts)
    assert np.abs(a["to_voxel"]).sum() > 0 and np.isfinite(a["to_voxel"]).all()
    assert np.array_equal(a["to_voxel"], b["to_voxel"])
    sets = [(a["list"], b["list"], plain["list"], perms[0])] + [(a["window"][k], b["window"][k], plain["window"][k], perms[k]) for k in range(P3)]
    for da, db, dp, pp in sets:
        assert set(da) == set(dp) == {"event_cnt", "event_mask", "event_voxel", "event_list_pol_mask"}
        assert np.abs(da["event_voxel"]).sum() > 0 and np.isfinite(da["event_voxel"]).all()
        assert np.array_equal(da["event_voxel"], db["event_voxel"])
        for k in ("event_cnt", "event_mask", "event_list_pol_mask"):
            assert np.array_equal(da[k], dp[k]), k
        assert np.array_equal(db["event_cnt"], dp["event_cnt"]) and np.array_equal(db["event_mask"], dp["event_mask"])
        for s, p in enumerate(pp):  # permuted row j holds original row p[j]
            assert np.array_equal(db["event_list_pol_mask"][s], dp["event_list_pol_mask"][s][p])
    # the window call bins pass k like the list call bins it, and the single-sample call like sample 0 of the batch
    assert np.array_equal(a["window"][0]["event_voxel"], a["list"]["event_voxel"])
    assert np.array_equal(a["to_voxel"], a["list"]["event_voxel"][0])


# ------------------------------------------------------------------ 2: order independence, IWE
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_2_iwe_images_do_not_depend_on_the_order_of_the_events(name, det_on):
    """compute_pol_iwe / deblur_events (bilinear), and a three-pass record through RSAT (nch = 4, timestamps), FWL,
    compute_window_iwe(round_idx=False) and compute_window_events, with per-pass flow maps and with overwrite_intermediate_flow:
    images and metric values bit for bit under a permutation within the pass segments (weights permuted alongside)."""
    win, other, _ = window(name)
    a, b = results("pol_iwes", name, True, False), pol_iwes(other, False)
    for k in a:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).sum() > 0, k
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))
    for overwrite in (False, True):
        a, b = results("metrics", name, True, overwrite), metrics(other, overwrite)
        for k in a:
            assert np.isfinite(a[k]).all() and np.abs(a[k]).sum() > 0, (k, overwrite)
            assert np.array_equal(a[k], b[k]), (k, overwrite, float(np.abs(a[k] - b[k]).max()))
        if name == "leaving":  # (events did leave: less mass in the image than events)
            assert float(a["window_iwe_bilinear"].sum()) < 0.9 * P3 * win["B"] * win["n"]


def test_2_empty_inputs(det_on):
    """No events at all (garbage in the output buffers beforehand), and a pass that holds padding (p = 0) only."""
    B, H, W = 2, 24, 40
    lib, st = _lib.load(), _lib.stream_ptr()
    fl = torch.zeros(B, 2, H, W, device=DEV)
    out = torch.full((B, 4, H, W), float("nan"), device=DEV)
    assert lib.evf_iwe_splat_det(fl.data_ptr(), None, None, None, None, None, 1, B, 0, H, W, 64.0, 1.0, 0.0, 4, 4, 1.0, out.data_ptr(), st) == EVF_OK
    dense = torch.full((B * P3 * (2 + 5 + 1) * H * W,), float("nan"), device=DEV)
    assert lib.evf_encode_window_det(None, B, P3, 0, H, W, 5, 0, 7, dense.data_ptr(), None, st) == EVF_OK
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(dense.abs().sum()) == 0
    z = hiwe.deblur_events(fl, torch.zeros(B, 0, 4, device=DEV), (H, W), round_idx=False)
    assert tuple(z.shape) == (B, 1, H, W) and float(z.abs().sum()) == 0
    win = make_window("stripes", empty=1)
    other, _ = permuted(win)
    many = enc.encode_window(G(np.stack(win["ev"], 1)), 5, (H, W))
    many2 = enc.encode_window(G(np.stack(other["ev"], 1)), 5, (H, W))
    assert float(many[1]["event_voxel"].abs().sum()) == 0 and float(many[0]["event_voxel"].abs().sum()) > 0
    for d, d2 in zip(many, many2):
        assert torch.equal(d["event_voxel"], d2["event_voxel"])
    a, b = metrics(win, False), metrics(other, False)
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    with mode(False):
        plain = metrics(win, False)
    assert np.array_equal(a["window_events"], plain["window_events"])


# ------------------------------------------------------------------ 3: the goldens at the project's bars
def test_3_encodings_golden(det_on):
    """g1_encodings at the bars of test_encodings_golden_bit_exact: rounded bit for bit, fractional atol 2e-6."""
    g = load_golden("g1_encodings")
    xs, ys, ts, ps = (G(g[k]) for k in ("xs", "ys", "ts", "ps"))
    res = tuple(int(v) for v in g["sensor"])
    for nb in (2, 5):
        got = N(enc.events_to_voxel(xs, ys, ts, ps, nb, sensor_size=res, round_ts=True))
        assert np.array_equal(got, g[f"voxel_nb{nb}_r1"])
        got = N(enc.events_to_voxel(xs, ys, ts, ps, nb, sensor_size=res, round_ts=False))
        np.testing.assert_allclose(got, g[f"voxel_nb{nb}_r0"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("tag", ["c1", "b2"])
@pytest.mark.parametrize("S", [128, 32])
def test_3_pol_iwe_golden(tag, S, det_on):
    """g3_pol_iwe at the bars of test_compute_pol_iwe_golden: rounded bit for bit, bilinear atol 3e-6."""
    g = load_golden("g3_pol_iwe")
    ev, flow, pol = G(g[tag + "_events"]), G(g[tag + "_flow"]), G(g[tag + "_pol"])
    res = tuple(int(v) for v in g[tag + "_res"])
    got = hiwe.compute_pol_iwe(flow, ev, res, pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=S, round_idx=True)
    assert np.array_equal(N(got), g[f"{tag}_iwe_s{S}_r1"])
    got = hiwe.compute_pol_iwe(flow, ev, res, pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=S, round_idx=False)
    np.testing.assert_allclose(N(got), g[f"{tag}_iwe_s{S}_r0"], rtol=0, atol=3e-6)


@pytest.mark.parametrize("ow", [0, 1])
def test_3_metrics_golden(ow, det_on):
    """g5_metrics at the bars of test_metrics_golden: FWL / RSAT rtol 1e-5, window images bit for bit."""
    g = load_golden("g5_metrics")
    H, W = (int(v) for v in g["res"])
    tag = f"ow{ow}"
    c = cfg(H, W, overwrite=bool(ow))
    ms = [hloss.FWL(c, DEV, flow_scaling=32), hloss.RSAT(c, DEV, flow_scaling=32)]
    last = None
    for k in range(int(g["P"])):
        last = G(g[f"{tag}_p{k}_flow"])
        inputs = {"event_list": G(g[f"{tag}_p{k}_event_list"]), "event_list_pol_mask": G(g[f"{tag}_p{k}_event_list_pol_mask"]),
                  "event_mask": G(g[f"{tag}_p{k}_event_mask"]), "gtflow": G(g[f"{tag}_p{k}_gtflow"]),
                  "dt_input": torch.tensor([1.0]), "dt_gt": torch.tensor([1.0])}
        for m in ms:
            m.event_flow_association([last], inputs)
    if ow:
        for m in ms:
            m.overwrite_intermediate_flow([last])
    np.testing.assert_allclose(N(ms[0]()), g[tag + "_fwl"], rtol=1e-5)
    np.testing.assert_allclose(N(ms[1]()), g[tag + "_rsat"], rtol=1e-5)
    assert np.array_equal(N(ms[0].compute_window_events()), g[tag + "_window_events"])
    assert np.array_equal(N(ms[0].compute_window_iwe()), g[tag + "_window_iwe"])


# ------------------------------------------------------------------ 4: against the default path
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_4_deterministic_path_matches_the_default_path(name):
    """The same per-event terms summed another way: rounded count images bit for bit; fractional voxels within atol 1e-5, bilinear
    and timestamp images within atol 2e-5 (the path-against-path bars of test_gpu_events.py)."""
    figures = []
    for nb in (2, 5):
        d, p = results("voxels", name, True, nb, False), results("voxels", name, False, nb, False)
        pairs = [(d["to_voxel"], p["to_voxel"]), (d["list"]["event_voxel"], p["list"]["event_voxel"])]
        pairs += [(d["window"][k]["event_voxel"], p["window"][k]["event_voxel"]) for k in range(P3)]
        figures.append((f"voxel nb{nb}", max(float(np.abs(x - y).max()) for x, y in pairs), 1e-5))
        d, p = results("voxels", name, True, nb, True), results("voxels", name, False, nb, True)
        assert np.array_equal(d["list"]["event_voxel"], p["list"]["event_voxel"])  # (rounded times: integer-valued)
    d, p = results("pol_iwes", name, True, True), results("pol_iwes", name, False, True)
    for k in d:
        assert np.array_equal(d[k], p[k]), k
    d, p = results("pol_iwes", name, True, False), results("pol_iwes", name, False, False)
    figures += [(k, float(np.abs(d[k] - p[k]).max()), 2e-5) for k in d]
    for overwrite in (False, True):
        d, p = results("metrics", name, True, overwrite), results("metrics", name, False, overwrite)
        for k in ("window_events", "window_iwe"):
            assert np.array_equal(d[k], p[k]), (k, overwrite)
        assert np.array_equal(d["ts_images"][:, 0:2], p["ts_images"][:, 0:2])
        figures += [(f"{k} ow{int(overwrite)}", float(np.abs(d[k] - p[k]).max()), 2e-5) for k in ("ts_images", "ts_images_bilinear", "window_iwe_bilinear")]
    print(name, [(k, f"{v:.3e}") for k, v, _ in figures])
    for k, v, bar in figures:
        assert v <= bar, (name, k, v, bar)


# ------------------------------------------------------------------ 5: known answers, exact in fp32
def test_5_known_answers_exact_in_fp32(det_on):
    """Event times in multiples of 1/8 (nb = 5: temporal weights 0, 1/2, 1), flows in multiples of 2^-6 (so of 2^-9) with
    flow_scaling 128 (warped coordinates in multiples of 1/4, bilinear weights of 1/4, timestamp terms of 2^-7), polarities +-1
    with both signs on the same pixels: every term and every partial sum is exact in fp32 in any order and with or without FMA
    contraction, so the outputs must EQUAL the oracle's and a float64 evaluation cast to float32 -- scaling, signs, layout."""
    B, n, H, W = 3, 900, 37, 53
    rng = np.random.default_rng(21)
    ev = np.empty((B, n, 4), np.float32)
    ev[:, :, 0] = rng.integers(0, 9, size=(B, n)) / 8.0
    ev[:, :, 1] = rng.integers(0, H, size=(B, n))
    ev[:, :, 2] = rng.integers(0, 12, size=(B, n)) + 20  # few columns: both polarities meet on the same pixels
    ev[:, :, 3] = rng.integers(0, 2, size=(B, n)) * 2 - 1
    pol = np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], 2).astype(np.float32)
    flow = (rng.integers(-12, 13, size=(B, 2, H, W)) / 64.0).astype(np.float32)
    # voxel: all three calls, both layouts
    ref64 = voxel_f64(ev, 5, H, W, False)
    assert (ref64 > 0).any() and (ref64 < 0).any() and np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64)
    d = enc.encode_event_list(G(ev), 5, (H, W))
    assert np.array_equal(N(d["event_voxel"]), ref64.astype(np.float32))
    for b in range(B):
        o = oenc.events_to_voxel(ev[b, :, 2], ev[b, :, 1], ev[b, :, 0], ev[b, :, 3], 5, (H, W))
        assert np.array_equal(N(d["event_voxel"][b]), o)
        e = G(ev[b])
        assert np.array_equal(N(enc.events_to_voxel(e[:, 2], e[:, 1], e[:, 0], e[:, 3], 5, sensor_size=(H, W))), o)
    evw = np.stack([ev, ev[:, ::-1], np.roll(ev, 7, 0)], 1)  # [B,P,n,4]
    many = enc.encode_window(G(evw), 5, (H, W))
    for k in range(P3):
        assert np.array_equal(N(many[k]["event_voxel"]), voxel_f64(evw[:, k], 5, H, W, False).astype(np.float32))
    # IWE: per-polarity bilinear images against the oracle, all four channels against float64
    gpol = G(pol)
    got = N(hiwe.compute_pol_iwe(G(flow), G(ev), (H, W), gpol[:, :, 0:1], gpol[:, :, 1:2], flow_scaling=128, round_idx=False))
    assert np.array_equal(got, oiwe.compute_pol_iwe(flow, ev, (H, W), pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=128, round_idx=False))
    got = N(hiwe.deblur_events(G(flow), G(ev), (H, W), flow_scaling=128, round_idx=False))
    assert np.array_equal(got, oiwe.deblur_events(flow, ev, (H, W), 128, False))
    sgn = pol[:, :, 0] - pol[:, :, 1]  # one signed plane: +1 and -1 land on the same pixels and cancel exactly
    for rnd in (False, True):
        ref64 = iwe_f64(flow, ev, H, W, 128.0, 1.0, sgn, pol[:, :, 1], 4, rnd)
        assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64) and (ref64[:, 0] < 0).any() and (ref64[:, 0] > 0).any()
        got = N(hiwe.iwe_splat(G(flow), G(ev), (H, W), 128, 1.0, round_idx=rnd, w0=G(sgn), w1=G(pol[:, :, 1]), nch=4, with_ts=True))
        assert np.array_equal(got, ref64.astype(np.float32)), rnd


def test_5_default_stripe_kernel_equals_the_exact_sum_kernel():
    """k_iwe_splat_lds against k_iwe_splat_det bit for bit where the sums are fractional: the dyadic inputs of the test above at
    B x n = 32 x 12517 = 400544 events (>= 400000: the default call takes the stripe kernel; n is no multiple of 4 x 1024: the
    clamped tail batch runs; 37 rows: stripes of 5 and a last one of 2).  12517 terms of at most 21 significant bits: every partial
    sum is exact in fp32 -- the float64 evaluation is its own fp32 rounding --, so the float atomics have no order to depend on and
    default == deterministic == float64, signed weights, four planes, rounded and bilinear."""
    B, n, H, W = 32, 12517, 37, 53
    rng = np.random.default_rng(22)
    ev = np.empty((B, n, 4), np.float32)
    ev[:, :, 0] = rng.integers(0, 9, size=(B, n)) / 8.0
    ev[:, :, 1] = rng.integers(0, H, size=(B, n))
    ev[:, :, 2] = rng.integers(0, 12, size=(B, n)) + 20
    pm = rng.integers(0, 2, size=(B, n)) * 2 - 1
    sgn, neg = pm.astype(np.float32), (pm < 0).astype(np.float32)
    flow = (rng.integers(-12, 13, size=(B, 2, H, W)) / 64.0).astype(np.float32)
    gf, ge, g0, g1 = G(flow), G(ev), G(sgn), G(neg)
    for rnd in (False, True):
        ref64 = iwe_f64(flow, ev, H, W, 128.0, 1.0, sgn, neg, 4, rnd)
        assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64)
        assert (ref64[:, 0] < 0).any() and (ref64[:, 0] > 0).any() and (ref64[:, :, 35:] != 0).any()  # (the short last stripe too)
        out = {}
        for on in (False, True):
            with mode(on):
                out[on] = N(hiwe.iwe_splat(gf, ge, (H, W), 128, 1.0, round_idx=rnd, w0=g0, w1=g1, nch=4, with_ts=True))
        assert np.array_equal(out[False], out[True]), rnd
        assert np.array_equal(out[True], ref64.astype(np.float32)), rnd


# ------------------------------------------------------------------ 6: accuracy against float64
def test_6_accuracy_against_float64_is_that_of_the_default_path():
    """Voxel grids and bilinear images (counts and timestamps) of two windows evaluated in float64; the default and the deterministic
    path are fp32 evaluations of identical per-event terms and differ in how the sums round, so the deterministic path's max-norm
    error may be at most twice the default path's error of this same run, plus 1e-9 (the rule of
    test_accuracy_against_float64_is_that_of_the_default_path).  The figures go to profiles/deterministic_splats_report.txt."""
    lines = ["deterministic voxel binning and IWE splats against a float64 evaluation of the oracle's formulas; max-norm errors of the",
             "default (float atomics) and the deterministic path", ""]
    bad = []
    for name in ("stripes", "ragged"):
        win = window(name)[0]
        (B, H, W, n), _ = GEOMETRY[name]
        S = float(max(H, W))
        ev, pol, fl = win["ev"][0], win["pol"][0], win["flows"][0]
        rows = [("voxel nb=5", voxel_f64(ev, 5, H, W, False),
                 lambda: N(enc.encode_event_list(G(ev), 5, (H, W))["event_voxel"])),
                ("bilinear IWE, 4 planes", iwe_f64(fl, ev, H, W, S, 1.0, pol[:, :, 0], pol[:, :, 1], 4, False),
                 lambda: N(hiwe.iwe_splat(G(fl), G(ev), (H, W), S, 1.0, round_idx=False, w0=G(pol[:, :, 0]), w1=G(pol[:, :, 1]), nch=4,
                                          with_ts=True)))]
        lines.append(f"{name} (B,H,W,n)={(B, H, W, n)}")
        for what, ref, run in rows:
            with mode(False):
                ep = float(np.abs(run().astype(np.float64) - ref).max())
            with mode(True):
                ed = float(np.abs(run().astype(np.float64) - ref).max())
            lines.append(f"  {what:24s} default {ep:.3e}  deterministic {ed:.3e}")
            print(lines[-1])
            if not ed <= 2.0 * ep + 1e-9:
                bad.append((name, what, ed, ep))
    with open(os.path.join(ROOT, "profiles", "deterministic_splats_report.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not bad, bad


# ------------------------------------------------------------------ 7: refusals
def test_7_refusals_precede_any_launch(det_on):
    lib, st = _lib.load(), _lib.stream_ptr()
    t = torch.full((64,), 7.0, device=DEV)
    ti = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    p, pi = t.data_ptr(), ti.data_ptr()

    def splat(M, H, W, nch=1, tau=1.0, out=p, flow=p, mode_=0, B=1):
        return lib.evf_iwe_splat_det(flow, p, pi, pi, p, p, 1, B, M, H, W, 64.0, 1.0, 0.0, mode_ | (4 if nch == 4 else 0), nch, tau, out, st)

    def events(N_, H, W, nb, voxel=p, B=1):
        return lib.evf_encode_events_det(p, B, N_, H, W, nb, 0, p, p, voxel, p, st)

    def win(N_, H, W, nb, want=7, dense=p, B=1, P=1):
        return lib.evf_encode_window_det(p, B, P, N_, H, W, nb, 0, want, dense, p, st)

    # a stripe row of more than 16384 slots
    assert splat(16, 1, 16385) == EVF_ENOTSUP and splat(16, 1, 8193, nch=2) == EVF_ENOTSUP and splat(16, 1, 4097, nch=4) == EVF_ENOTSUP
    assert splat(16, 1, 16385, mode_=1) == EVF_ENOTSUP
    assert events(16, 1, 3277, 5) == EVF_ENOTSUP and win(16, 1, 3277, 5) == EVF_ENOTSUP and events(16, 1, 16385, 1) == EVF_ENOTSUP
    # so many events, or so large a timestamp bound, that k < 32
    assert splat(1 << 30, 8, 8) == EVF_ENOTSUP and splat(1 << 20, 8, 8, nch=4, tau=1024.0) == EVF_ENOTSUP
    assert events(1 << 30, 8, 8, 2) == EVF_ENOTSUP and win(1 << 30, 8, 8, 2) == EVF_ENOTSUP
    assert lib.evf_splat_det_bits(1 << 30, 1.0) == EVF_ENOTSUP and lib.evf_splat_det_bits((1 << 30) - 1, 1.0) == 32
    # more samples than a grid holds
    assert splat(16, 8, 8, B=65536) == EVF_ENOTSUP and win(16, 8, 8, 2, B=256, P=256) == EVF_ENOTSUP
    # bad pointers and shapes
    assert splat(16, 8, 8, out=None) == EVF_EINVAL and splat(16, 8, 8, flow=None) == EVF_EINVAL and splat(16, 8, 8, nch=3) == EVF_EINVAL
    assert splat(16, 0, 8) == EVF_EINVAL and splat(16, 8, 8, nch=4, tau=float("nan")) == EVF_EINVAL
    assert lib.evf_iwe_splat_det(p, p, pi, pi, p, p, 1, 1, 16, 8, 8, 64.0, 1.0, 0.0, 0, 4, 1.0, p, st) == EVF_EINVAL  # nch 4 without mode 4
    assert events(16, 8, 0, 2) == EVF_EINVAL and events(16, 8, 8, 0) == EVF_EINVAL and win(16, 8, 8, 2, dense=None) == EVF_EINVAL
    assert lib.evf_encode_events_det(None, 1, 16, 8, 8, 2, 0, p, p, p, p, st) == EVF_EINVAL
    torch.cuda.synchronize()
    assert float((t - 7.0).abs().sum()) == 0 and int((ti - 7).abs().sum()) == 0  # nothing ran
    # the Python wrappers say why, and do not fall back to the atomics
    _lib.profile_start(NAMES6)
    e = G(synthetic.event_list_batch(1, 50, 2, 3277, 1))
    with pytest.raises(_lib.EvflowError, match="16384"):
        enc.events_to_voxel(e[0, :, 2], e[0, :, 1], e[0, :, 0], e[0, :, 3], 5, sensor_size=(2, 3277))
    with pytest.raises(_lib.EvflowError, match="16384"):
        enc.encode_event_list(e, 5, (2, 3277))
    with pytest.raises(_lib.EvflowError, match="16384"):
        enc.encode_window(e.view(1, 1, 50, 4), 5, (2, 3277))
    e = G(synthetic.event_list_batch(1, 50, 2, 8193, 1))
    pol = torch.stack([(e[:, :, 3] > 0).float(), (e[:, :, 3] < 0).float()], 2).contiguous()
    with pytest.raises(_lib.EvflowError, match="16384"):
        hiwe.compute_pol_iwe(torch.zeros(1, 2, 2, 8193, device=DEV), e, (2, 8193), pol[:, :, 0:1], pol[:, :, 1:2], round_idx=False)
    assert not any(v for v in _lib.profile_stop().values())  # no entry point ran, the default ones neither
    # one column fewer is served
    ok = hiwe.compute_pol_iwe(torch.zeros(1, 2, 2, 8192, device=DEV), G(synthetic.event_list_batch(1, 50, 2, 8192, 1)), (2, 8192),
                              pol[:, :, 0:1], pol[:, :, 1:2], round_idx=False)
    assert float(ok.sum()) == 50.0


# ------------------------------------------------------------------ 8: routing
def _seen(fn):
    _lib.profile_start(NAMES6)
    fn()
    return {k[0] for k, v in _lib.profile_stop().items() if v}


def test_8_the_switch_selects_the_entry_points():
    win = window("stripes")[0]
    B, H, W = win["B"], win["H"], win["W"]

    def binning():
        voxels(win, 5, False)

    def images():
        pol_iwes(win, False)
        pol_iwes(win, True)
        metrics(win, False)

    def counts_only():
        enc.encode_event_list(G(win["ev"][0]), 2, (H, W), want=("cnt", "mask", "pol"))
        enc.encode_window(G(np.stack(win["ev"], 1)), 2, (H, W), want=("cnt", "mask", "pol"))
        lists = G(np.stack(win["ev"], 1))
        enc.encode_event_lists([lists[:, k] for k in range(P3)], 2, (H, W), want=("cnt", "mask", "pol"))

    with mode(False):
        assert _seen(binning) == {"evf_encode_events", "evf_encode_window"}
        assert _seen(images) == {"evf_iwe_splat"}
        assert _seen(counts_only) == {"evf_encode_events", "evf_encode_window"}
    with mode(True):
        assert _seen(binning) == {"evf_encode_events_det", "evf_encode_window_det"}
        assert _seen(images) == {"evf_iwe_splat_det"}
        assert _seen(counts_only) == {"evf_encode_events", "evf_encode_window"}  # no voxel grid requested: the default call
        lists = G(np.stack(win["ev"], 1))
        assert _seen(lambda: enc.encode_event_lists([lists[:, k] for k in range(P3)], 5, (H, W))) == {"evf_encode_window_det"}
