"""The yardstick of evf_render_sheet (tests/render_ref.py) checked without a device: the percentile positions against
np.percentile bit for bit, the restatement against utils/visualization.py and fixture G17 on the inputs of tests/test_gpu_render.py,
the host guards of --render device, and the kernel launcher's guards as a stand-alone program under the host sanitizers."""

import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import render_ref as R
from event_flow_amd import _lib
from event_flow_amd.utils import visualization as vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


@pytest.mark.parametrize("n", [2, 6, 35, 2145])
def test_percentile_position_and_lerp_are_np_percentile_bit_for_bit(n):
    r = np.random.default_rng(n)
    arrays = {"distinct": r.normal(0.3, 2.0, n), "ties": r.poisson(0.7, n).astype(F64), "steps": np.repeat(r.normal(0, 1, (n + 2) // 3), 3)[:n],
              "negative fractions": -np.abs(r.normal(0, 1e-3, n))}
    weights = []
    for p in (1, 99, 0, 100, 50, 30, 75, 12.5, 99.9):
        k, g = vis.percentile_position(n, p)
        assert 0 <= k <= n - 1 and 0.0 <= g < 1.0
        weights.append(g)
        for name, x in arrays.items():
            s = np.sort(x)
            mine = R.lerp(s[k], s[min(k + 1, n - 1)], g)
            assert mine.tobytes() == np.percentile(x, p).tobytes(), (name, n, p, k, g)
            assert R.percentile(x, p).tobytes() == np.percentile(x, p).tobytes()
    assert any(0 < g < 0.5 for g in weights) and any(g >= 0.5 for g in weights)  # both branches of the lerp


def test_the_distinct_counts_interpolate_on_both_sides_of_one_half():
    """The `distinct` content of the GPU test: order statistics k and k + 1 differ at both positions, with weights below and from
    0.5 on across the shapes."""
    below = above = 0
    for H, W in R.SHAPES:
        n = H * W
        for p in (1, 99):
            k, g = vis.percentile_position(n, p)
            for ch in R.count_image("distinct", H, W, 0):
                s = np.sort(ch.ravel())
                if k + 1 < n and g > 0:
                    assert s[k] != s[k + 1]
                    below += g < 0.5
                    above += g >= 0.5
    assert below and above
    assert vis.percentile_position(2, 1) == (0, pytest.approx(0.01)) and vis.percentile_position(2, 99)[1] >= 0.5


def _host_u8(x, scheme):
    """events_to_image(...) * 255 -> _u8 of a [2,H,W] image, in PNG channel order (Visualization._events_png)."""
    img = vis.events_to_image(np.asarray(x).transpose(1, 2, 0), scheme) * 255
    return vis._u8(img[:, :, ::-1]) if img.ndim == 3 else np.repeat(vis._u8(img)[:, :, None], 3, 2)


@pytest.mark.parametrize("scheme", R.SCHEMES)
def test_counts_restatement_equals_events_to_image(scheme):
    g = R.g17()
    for k in range(3):
        cnt = g[f"cnt{k}"]
        assert np.array_equal(cnt, cnt.astype(np.float32))  # (exact in float32, the device's input type)
        x = cnt.transpose(2, 0, 1).astype(np.float32)
        u8, pre = R.counts(x, scheme)
        assert np.array_equal(u8, _host_u8(x, scheme))
        ref = g[f"cnt{k}_green_red"][:, :, ::-1] if scheme == "green_red" else np.repeat(g[f"cnt{k}_gray"][:, :, None], 3, 2)
        np.testing.assert_allclose(pre, ref * 255, rtol=0, atol=255e-12)  # the reference's own events_to_image
    for H, W in R.SHAPES:
        for B in (1, 3):
            for content in R.COUNT_CONTENTS:
                if (H, W) == (180, 240) and (B, content) not in ((1, "poisson"), (3, "fractional")):
                    continue  # (the large shape: the two cases the GPU test runs)
                u8, _pre = R.count_ref(content, H, W, B, scheme)
                for b, x in enumerate(R.count_batch(content, H, W, B)):
                    assert np.array_equal(u8[b], _host_u8(x, scheme)), (content, H, W, B, b)


def test_count_contents_are_what_they_claim():
    H, W = 33, 65
    assert not R.count_image("zero", H, W, 0).any()
    s = R.count_image("single", H, W, 0)
    assert s[0].any() and not s[1].any()
    assert (R.count_image("const3", H, W, 0) == 3.0).all()
    p = R.count_image("poisson", H, W, 0)
    assert (p == 0).mean() > 0.6 and p.max() >= 2  # heavy ties
    d = R.count_image("distinct", H, W, 0)
    assert all(np.unique(c).size == H * W for c in d)
    f = R.count_image("fractional", H, W, 0)
    assert (f < 0).any() and (f % 1 != 0).all()
    three = R.count_batch("zero", 5, 7, 3)
    assert not three[0].any() and three[1].any() and not np.array_equal(three[1], three[2])  # different content per sample


def test_flow_restatement_holds_the_g17_bar_on_the_gpu_tests_inputs():
    g = R.g17()
    u8, _ = R.flow_ref("g17")
    for k in range(4):
        worst, share = R.g17_bar(u8[k], g[f"flow{k}_rgb"])
        assert worst <= 1 and share < 0.01, (k, worst, share)
    for name, batch in R.flow_inputs().items():
        u8, pre = R.flow_ref(name)
        for b, f in enumerate(batch):
            worst, share = R.g17_bar(u8[b], vis.flow_to_image(f[0], f[1]))  # the float32 host renderer
            assert worst <= 1 and share < 0.01, (name, b, worst, share)
            band = np.abs(pre[b] - np.rint(pre[b])) <= 1e-6  # where the GPU test allows one level
            exact = (pre[b] == 0.0) | (pre[b] == 255.0)       # p = 0 and val = 1: the same bits on any IEEE machine
            assert (band & ~exact).mean() < 0.01, (name, b)
    n = R.flow_inputs()
    for name in ("normal_1", "normal_davis"):
        mag = np.hypot(*n[name][0].astype(F64))
        assert mag.max() - mag.min() >= 1.0
    assert not n["zero_1"].any() and np.ptp(np.hypot(*n["const_1"][0].astype(F64))) == 0.0 and n["const_1"].any()
    sz = n["signed_zero_1"][0]
    assert ((sz == 0) & np.signbit(sz)).any() and ((sz == 0) & ~np.signbit(sz)).any() and (sz != 0).any()
    ax = n["axis_1"][0]
    assert ((ax[0] == 0) | (ax[1] == 0)).all() and (ax[0] > 0).any() and (ax[0] < 0).any() and (ax[1] > 0).any() and (ax[1] < 0).any()


def test_render_device_refusals_need_no_device(tmp_path, monkeypatch):
    import yaml

    import eval_flow
    from event_flow_amd.configs.parser import YAMLParser

    ns = types.SimpleNamespace
    assert eval_flow.render_refusal(ns(store="out"), "cpu") is None  # (hand-made args without the newer flag: host)
    assert eval_flow.render_refusal(ns(store="", render="host"), "cpu") is None
    assert eval_flow.render_refusal(ns(store="out", render="device"), "cuda:0") is None
    why = eval_flow.render_refusal(ns(store="", render="device"), "cuda:0")
    assert "--store" in why and "drop --render device" in why
    why = eval_flow.render_refusal(ns(store="out", render="device"), "cpu")
    assert "CUDA device" in why and "--render host" in why
    assert "host or device" in eval_flow.render_refusal(ns(store="out", render="png"), "cuda:0")

    def no_device(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.nn.Module, "to", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    tcfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_SNN.yml")))
    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    yaml.safe_dump(tcfg, open(tmp_path / "train.yml", "w"))
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))

    def run(match, **kw):
        args = ns(train_config=str(tmp_path / "train.yml"), weights="", sequences=2, resident=False, graphed=False, synthetic=True,
                  per_sequence=False, **kw)
        parser = YAMLParser(str(tmp_path / "eval.yml"))
        if kw.get("cpu"):
            parser._device = torch.device("cpu")
        with pytest.raises(_lib.EvflowError, match=match):
            eval_flow.test(args, parser)

    run("add --store", store="", render="device")
    run("use --render host", store=str(tmp_path / "png"), render="device", cpu=True)
    # --graphed --store stays refused, whatever the renderer
    args = ns(train_config=str(tmp_path / "train.yml"), weights="", sequences=2, resident=True, graphed=True, synthetic=False,
              per_sequence=False, store=str(tmp_path / "png"), render="device")
    with pytest.raises(_lib.EvflowError, match="use --store"):
        eval_flow.test(args, YAMLParser(str(tmp_path / "eval.yml")))
    assert not (tmp_path / "png").exists()

    with pytest.raises(ValueError, match="host or device"):
        vis.Visualization({}, eval_id=0, path_results=str(tmp_path) + "/", render="gpu")
    cpu = torch.zeros(1, 2, 4, 4)
    with pytest.raises(_lib.EvflowError, match="no CPU fallback"):
        vis.render_sheet([(vis.RENDER_COUNTS, cpu)])
    with pytest.raises(_lib.EvflowError, match="1 to 8 images"):
        vis.render_sheet([])
    with pytest.raises(_lib.EvflowError, match="1 to 8 images"):
        vis.render_sheet([(vis.RENDER_COUNTS, cpu)] * 9)
    with pytest.raises(_lib.EvflowError, match="colour scheme"):
        vis.render_sheet([(vis.RENDER_COUNTS, cpu)], scheme="blue")


def test_launcher_guards_as_a_sanitized_stand_alone_program(tmp_path):
    """tools/render_guards.cpp with csrc/evf_render.hip, host code under AddressSanitizer and UBSan: every EVF_EINVAL case is
    answered before any launch (the program makes no accepted call, so it never launches)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc to build tools/render_guards.cpp with")
    exe = str(tmp_path / "render_guards")
    cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "event_flow_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "render_guards.cpp"), os.path.join(ROOT, "event_flow_amd", "csrc", "evf_render.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
    assert "all guards answered EVF_EINVAL before any launch" in ran.stdout
