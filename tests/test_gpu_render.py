"""evf_render_sheet (csrc/evf_render.hip) on the MI355X against the float64 restatement of tests/render_ref.py (pinned to
utils/visualization.py and fixture G17 by tests/test_host_render_reference.py): count images byte for byte, flow images at the
derived rule and at the G17 bar, frames exactly, a mixed sheet between canaries, call-to-call and replayed bits, every host guard,
and Visualization(render="device") / eval_flow.py --render device on top of it."""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R
from event_flow_amd import _lib
from event_flow_amd.utils import visualization as vis

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def one(kind, batch, scheme="green_red"):
    """The sheet of a single image kind: uint8 [B,H,W,3] on the host."""
    out = vis.render_sheet([(kind, dev(batch))], scheme)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == (batch.shape[0], 1) + batch.shape[2:] + (3,)
    return out.cpu().numpy()[:, 0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_counts_are_byte_equal(H, W, B):
    contents = R.COUNT_CONTENTS if (H, W) != (180, 240) else (("poisson",) if B == 1 else ("fractional",))
    for content in contents:
        for scheme in R.SCHEMES:
            want, _pre = R.count_ref(content, H, W, B, scheme)
            got = one(R.COUNTS, R.count_batch(content, H, W, B), scheme)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (content, scheme, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", sorted(R.flow_inputs()))
def test_flow_follows_the_derived_rule(name):
    """A channel equals the restatement wherever the restatement's 255 c lies more than 1e-6 from an integer (float64 atan2 and hypot
    of another libm move 255 c by about 1e-12); inside that band one level, and the band holds fewer than 1 % of an image."""
    want, pre = R.flow_ref(name)
    got = one(R.FLOW, R.flow_inputs()[name])
    band = np.abs(pre - np.rint(pre)) <= 1e-6
    d = np.abs(got.astype(int) - want.astype(int))
    print(name, "differing values", int((d > 0).sum()), "of", d.size, "in the band", int(band.sum()))
    assert not d[~band].any(), (name, np.argwhere((d > 0) & ~band)[:4].tolist())
    assert d.max() <= 1
    exact = (pre == 0.0) | (pre == 255.0)  # p = 0 and val = 1: the same bits on any IEEE machine, and they must agree
    assert not d[exact].any()
    for b in range(got.shape[0]):
        assert (band[b] & ~exact[b]).mean() < 0.01 and (d[b] > 0).mean() < 0.01, (name, b)


def test_flow_holds_the_g17_bar():
    g = R.g17()
    got = one(R.FLOW, R.flow_inputs()["g17"])
    for k in range(4):
        worst, share = R.g17_bar(got[k], g[f"flow{k}_rgb"])
        print("flow", k, "largest difference", worst, "share", share)
        assert worst <= 1 and share < 0.01, (k, worst, share)


@pytest.mark.parametrize("B,H,W", [(1, 1, 2), (3, 5, 7), (2, 33, 65), (1, 180, 240)])
def test_frames_are_copied_exactly(B, H, W):
    f = np.stack([R.frame_image(H, W, b) for b in range(B)])
    got = one(R.FRAME, f)
    for c in range(3):
        assert np.array_equal(got[..., c], f[:, 1])


class Sheet:
    """nimg = 5 images of mixed kinds for B = 3 samples of 33 x 65 pixels, called through ctypes into a buffer between canaries."""

    B, H, W, GUARD = 3, 33, 65, 4096

    def __init__(self):
        B, H, W = self.B, self.H, self.W
        self.kinds = [R.COUNTS, R.FLOW, R.FRAME, R.COUNTS, R.FLOW]
        self.host = [R.count_batch("poisson", H, W, B), np.stack([R.flow_image("normal", H, W, b) for b in range(B)]),
                     np.stack([R.frame_image(H, W, b) for b in range(B)]), R.count_batch("fractional", H, W, B),
                     np.stack([R.flow_image("signed_zero", H, W, b) for b in range(B)])]
        self.src = [dev(a) for a in self.host]
        self.bytes = B * 5 * H * W * 3
        self.full = torch.full((self.bytes + 2 * self.GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        (self.k_lo, self.g_lo), (self.k_hi, self.g_hi) = vis.percentile_position(H * W, 1), vis.percentile_position(H * W, 99)

    def args(self, pick=None, out=None):
        pick = list(range(5)) if pick is None else pick
        src = (ctypes.c_void_p * len(pick))(*[self.src[k].data_ptr() for k in pick])
        kinds = (ctypes.c_int * len(pick))(*[self.kinds[k] for k in pick])
        out = self.full.data_ptr() + self.GUARD if out is None else out
        return [src, kinds, len(pick), self.B, self.H, self.W, 0, self.k_lo, self.g_lo, self.k_hi, self.g_hi, out]

    def payload(self):
        torch.cuda.synchronize()
        full = self.full.cpu().numpy()
        assert (full[:self.GUARD] == 0xA5).all() and (full[-self.GUARD:] == 0xA5).all(), "a store outside the sheet"
        return full[self.GUARD:-self.GUARD].reshape(self.B, 5, self.H, self.W, 3).copy()


def test_sheet_of_mixed_kinds_between_canaries_call_to_call_and_replayed():
    s = Sheet()
    assert _lib.raw("evf_render_sheet", *s.args()) == 0
    first = s.payload()
    for k in range(5):  # every image equals the one of its own single-image call
        alone = torch.full((s.B, 1, s.H, s.W, 3), 0x5A, dtype=torch.uint8, device=DEV)
        assert _lib.raw("evf_render_sheet", *s.args([k], alone.data_ptr())) == 0
        assert np.array_equal(alone.cpu().numpy()[:, 0], first[:, k]), k
    assert np.array_equal(first[:, 0], R.count_ref("poisson", s.H, s.W, s.B, "green_red")[0])
    assert np.array_equal(first[:, 3], R.count_ref("fractional", s.H, s.W, s.B, "green_red")[0])
    assert np.array_equal(first[:, 2, :, :, 0], s.host[2][:, 1])
    s.full.fill_(0xA5)
    assert _lib.raw("evf_render_sheet", *s.args()) == 0
    assert np.array_equal(s.payload(), first)  # a second call: bit for bit
    s.full.fill_(0xA5)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        assert _lib.raw("evf_render_sheet", *s.args()) == 0
    torch.cuda.synchronize()
    assert (s.full == 0xA5).all()  # captured, not run
    for _ in range(2):
        s.full.fill_(0xA5)
        g.replay()
        assert np.array_equal(s.payload(), first)


def test_host_guards():
    s = Sheet()
    ok = s.args()
    assert _lib.raw("evf_render_sheet", *ok) == 0
    s.payload()
    s.full.fill_(0xA5)
    n = s.H * s.W
    nan = float("nan")

    def arr(kind, values):
        return (kind * len(values))(*values)

    ptrs = [t.data_ptr() for t in s.src]
    bad = [(0, None), (1, None), (11, None)]                                            # null src, kind, out
    bad += [(0, arr(ctypes.c_void_p, ptrs[:k] + [None] + ptrs[k + 1:])) for k in (0, 2, 4)]  # a null src[k]
    bad += [(2, v) for v in (0, -1, 9)]                                                 # nimg outside 1..8
    bad += [(1, arr(ctypes.c_int, [0, 1, v, 0, 1])) for v in (-1, 3, 7)]                # an unknown kind
    bad += [(6, v) for v in (-1, 2)]                                                    # an unknown scheme
    bad += [(k, v) for k in (3, 4, 5) for v in (0, -1)]                                 # a non-positive B, H, W
    bad += [(3, 13108), (3, 2 ** 31 - 1)]                                               # B nimg > 65535
    bad += [(7, -1), (7, n), (9, -1), (9, n), (9, 2 ** 31 - 1)]                         # k outside 0 .. H W - 1
    bad += [(8, 1.0), (8, -1e-9), (8, nan), (10, 1.0), (10, -0.25), (10, nan), (10, float("inf"))]  # g outside [0, 1)
    bad += [(0, arr(ctypes.c_void_p, [ptrs[0] + 2] + ptrs[1:])), (0, arr(ctypes.c_void_p, ptrs[:4] + [ptrs[4] + 1]))]  # misaligned floats
    for at, value in bad:
        args = list(ok)
        args[at] = value
        assert _lib.raw("evf_render_sheet", *args) == EINVAL, (at, value)
    # H W > 2^18 (the order statistics stay those of 33 x 65, in range for every size here: only the size is wrong)
    for H, W in ((513, 512), (1, 2 ** 18 + 1), (65536, 65536)):
        args = list(ok)
        args[4], args[5] = H, W
        assert _lib.raw("evf_render_sheet", *args) == EINVAL, (H, W)
    torch.cuda.synchronize()
    assert (s.full == 0xA5).all()  # no refused call stored anything
    # a frame may sit at any byte address; the last order statistic and a weight just below one are accepted
    odd = torch.zeros(s.B * 2 * n + 1, dtype=torch.uint8, device=DEV)
    odd[1:] = s.src[2].reshape(-1)
    args = s.args([2])
    args[0] = arr(ctypes.c_void_p, [odd.data_ptr() + 1])
    args[7], args[8], args[9], args[10] = n - 1, 0.0, n - 1, 1.0 - 2.0 ** -53
    assert _lib.raw("evf_render_sheet", *args) == 0
    torch.cuda.synchronize()
    full = s.full.cpu().numpy()
    tile = full[s.GUARD:s.GUARD + s.B * n * 3].reshape(s.B, s.H, s.W, 3)
    assert np.array_equal(tile[..., 1], s.host[2][:, 1]) and (full[s.GUARD + s.B * n * 3:] == 0xA5).all()
    with pytest.raises(_lib.EvflowError, match="like the first"):
        vis.render_sheet([(vis.RENDER_COUNTS, s.src[0]), (vis.RENDER_FLOW, torch.zeros(1, 2, 4, 5, device=DEV))])


# ---------------------------------------------------------------------------------------------------------------------------
# Visualization(render="device") and the driver
# ---------------------------------------------------------------------------------------------------------------------------
def _tree(base):
    return sorted(os.path.relpath(os.path.join(d, f), base) for d, _s, files in os.walk(base) for f in files)


def _pass(B, H, W, k, window):
    """The tensors of stored pass k: counts, flow, IWE, ground truth, frames, and the three window images on demand."""
    cnt = dev(np.stack([R.count_image("poisson", H, W, 10 * k + b) for b in range(B)]))
    iwe = dev(np.stack([R.count_image("fractional", H, W, 10 * k + b) for b in range(B)]))
    flow = dev(np.stack([R.flow_image("normal", H, W, 10 * k + b) for b in range(B)]))
    gt = dev(np.stack([R.flow_image("axis", H, W, 10 * k + b) for b in range(B)]))
    frames = dev(np.stack([R.frame_image(H, W, 10 * k + b) for b in range(B)]))
    win = (cnt * 2, flow * 0.5, iwe + 1) if window else (None, None, None)
    return {"event_cnt": cnt, "gtflow": gt, "frames": frames}, flow, iwe, win


def test_device_store_writes_the_host_tree_with_byte_equal_count_images(tmp_path):
    H, W = 33, 65
    stores = {r: vis.Visualization({}, eval_id=1, path_results=str(tmp_path / r) + "/", render=r) for r in ("host", "device")}
    for k in range(3):
        inputs, flow, iwe, win = _pass(1, H, W, k, window=k == 1)
        stores["host"].store(inputs, flow, iwe, "seqA", *win, ts=0.25 * k)
        stores["device"].store(inputs, flow, iwe, ["seqA"], *win, ts=0.25 * k)
    host, device = (str(tmp_path / r / "results" / "eval_1") for r in ("host", "device"))
    assert _tree(host) == _tree(device) and "seqA/events_window/000000001.png" in _tree(device) and len(_tree(device)) == 3 * 5 + 3 + 1
    for rel in _tree(host):
        same = open(os.path.join(host, rel), "rb").read() == open(os.path.join(device, rel), "rb").read()
        if rel.split("/")[1] in ("events", "events_window", "iwe", "iwe_window", "frames", "timestamps.txt"):
            assert same, rel  # (flow images: float64 on the device, float32 in numpy -- the G17 bar, above)


def test_device_store_keeps_a_folder_and_a_counter_per_slot(tmp_path):
    H, W = 16, 24
    v = vis.Visualization({}, eval_id=0, path_results=str(tmp_path) + "/", render="device")
    for k, folders in enumerate((["a", "b", "c"], ["a", "b", "c"], ["a", "b", "d"], ["c", "b", "a"])):  # (c is visited again)
        inputs, flow, iwe, _win = _pass(3, H, W, k, window=False)
        v.store(inputs, flow, iwe, folders, ts=float(k))
        if k == 0:
            want = [one(R.COUNTS, inputs["event_cnt"].cpu().numpy())[b] for b in range(3)]
    base = tmp_path / "results" / "eval_0"
    assert sorted(p.name for p in base.iterdir()) == ["a", "b", "c", "d"]
    count = {f: sorted(p.name for p in (base / f / "iwe").iterdir()) for f in "abcd"}
    assert count == {"a": ["%09d.png" % k for k in range(4)], "b": ["%09d.png" % k for k in range(4)],
                     "c": ["%09d.png" % k for k in range(3)], "d": ["000000000.png"]}
    assert (base / "a" / "timestamps.txt").read_text() == "0.0\n1.0\n2.0\n3.0\n" and (base / "d" / "timestamps.txt").read_text() == "2.0\n"
    assert (base / "c" / "timestamps.txt").read_text() == "0.0\n1.0\n3.0\n"  # the counter and the file go on where they stopped
    assert v._pinned.numel() == 3 * 8 * H * W * 3  # one pinned buffer, sized for eight images
    from test_host_visualization import _read_png

    for b, f in enumerate("abc"):  # every slot's own image
        assert np.array_equal(_read_png(base / f / "events" / "000000000.png"), want[b])
    with pytest.raises(ValueError, match="different folder names"):
        v.store(inputs, flow, iwe, ["a", "a", "b"])


def test_driver_stores_every_slot_and_the_window_images(tmp_path):
    """eval_flow.py --synthetic --store --render device in a fresh process, window_eval = 2 window, batch_size = 2: a folder per
    slot, and the three window images at every stored pass whose metric fired -- every second one."""
    import yaml

    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    ecfg["data"]["window_eval"] = 2 * ecfg["data"]["window"]
    ecfg["loader"]["batch_size"] = 2
    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_flow.py"), "--synthetic", "--sequences", "2", "--config",
                          str(tmp_path / "eval.yml"), "--store", str(tmp_path), "--render", "device"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert {"FWL", "RSAT"} <= set(res)
    base = tmp_path / "results" / "eval_0"
    assert sorted(p.name for p in base.iterdir()) == ["seq000_slot0", "seq000_slot1"]
    for slot in base.iterdir():
        passes = sorted(p.name for p in (slot / "events").iterdir())
        assert len(passes) == 20 and passes == sorted(p.name for p in (slot / "flow").iterdir()) == sorted(p.name for p in (slot / "iwe").iterdir())
        for sub in ("events_window", "flow_window", "iwe_window"):
            assert sorted(p.name for p in (slot / sub).iterdir()) == passes[1::2], sub  # the passes that closed a window
    a, b = (open(base / s / "iwe" / "000000003.png", "rb").read() for s in ("seq000_slot0", "seq000_slot1"))
    assert a != b  # two sequences, not one stored twice


def test_pinned_buffer_is_allocated_once_while_the_window_images_come_and_go(tmp_path):
    v = vis.Visualization({}, eval_id=0, path_results=str(tmp_path) + "/", render="device")
    where = set()
    for k in range(4):
        inputs, flow, iwe, win = _pass(2, 16, 24, k, window=k % 2 == 1)
        v.store(inputs, flow, iwe, ["a", "b"], *win)
        where.add(v._pinned.data_ptr())
    assert len(where) == 1 and v._pinned.is_pinned()
    base = tmp_path / "results" / "eval_0" / "b"
    assert sorted(p.name for p in (base / "iwe_window").iterdir()) == ["000000001.png", "000000003.png"]


def _driver(tmp_path, ecfg, *flags):
    import yaml

    yaml.safe_dump(ecfg, open(tmp_path / "eval.yml", "w"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_flow.py"), "--config", str(tmp_path / "eval.yml"), "--store",
                          str(tmp_path), *flags], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), tmp_path / "results" / "eval_0"


def test_driver_with_the_host_renderer_stores_the_window_images_too(tmp_path):
    """--render host at B = 1 and window_eval = 2 window: the store call sits behind the metric loop for both renderers."""
    import yaml

    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    ecfg["data"]["window_eval"] = 2 * ecfg["data"]["window"]
    _res, base = _driver(tmp_path, ecfg, "--synthetic", "--sequences", "1", "--render", "host")
    assert [p.name for p in base.iterdir()] == ["seq000"]
    passes = sorted(p.name for p in (base / "seq000" / "events").iterdir())
    assert passes == ["%09d.png" % k for k in range(20)]
    for sub in ("flow", "iwe"):
        assert sorted(p.name for p in (base / "seq000" / sub).iterdir()) == passes
    for sub in ("events_window", "flow_window", "iwe_window"):
        assert sorted(p.name for p in (base / "seq000" / sub).iterdir()) == passes[1::2], sub


SEQ_WINDOW, SEQ_WINDOWS = 1000, {"a": 2, "b": 6, "c": 2}  # windows per file: unequal lengths, a is opened a second time


def _visits(B):
    """The loaders' slot rule replayed on the host: folder -> (file, windows stored), in order of appearance.  A slot that has no
    whole window left restarts on sequence number max + 1, file number % len(files); the batch with the len(files)-th restart is
    the wrap-around one, which the driver drops."""
    files = sorted(SEQ_WINDOWS)
    idx, row, restarts, stored = list(range(B)), [0] * B, 0, {}
    while True:
        for b in range(B):
            while row[b] >= SEQ_WINDOWS[files[idx[b] % len(files)]]:
                restarts, idx[b], row[b] = restarts + 1, max(idx) + 1, 0
        if restarts >= len(files):
            return stored
        for b in range(B):
            f, visit = files[idx[b] % len(files)], idx[b] // len(files)
            folder = f + ("_visit%d" % visit if visit else "")
            stored.setdefault(folder, [f, 0])[1] += 1
            row[b] += 1


@pytest.mark.parametrize("loader", ["h5", "resident"])
def test_driver_on_sequence_files_files_every_pass_under_its_own_visit(tmp_path, loader):
    """B = 2 over three files of unequal length, H5Loader and --resident: slot 0 comes back to file a before the pass is over.
    Every folder holds exactly the windows of one visit of its file -- the first and the last stored count image are the
    file's own windows --, none is misfiled under the next file's name."""
    import yaml

    from event_flow_amd import synthetic
    from event_flow_amd.dataloader.h5 import write_npz_sequence
    from test_host_visualization import _read_png

    assert _visits(2) == {"a": ["a", 2], "b": ["b", 6], "c": ["c", 2], "a_visit1": ["a", 2]}
    H = W = 64
    data = tmp_path / "data"
    data.mkdir()
    events = {}
    for i, (name, windows) in enumerate(SEQ_WINDOWS.items()):
        n = windows * SEQ_WINDOW + 300  # (a remainder shorter than a window)
        xs, ys, ts, ps, _uv = synthetic.moving_dots_events(n, H, W, 500 + i, max_disp=30.0)
        events[name] = (np.asarray(xs).astype(int), np.asarray(ys).astype(int), np.asarray(ps) > 0)
        write_npz_sequence(str(data / f"{name}.npz"), xs.astype(np.int16), ys.astype(np.int16), ts + 5.0, (ps > 0).astype(np.int8))
    ecfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "eval_flow.yml")))
    ecfg["data"].update(path=str(data), mode="events", window=SEQ_WINDOW, window_eval=2 * SEQ_WINDOW)
    ecfg["loader"]["batch_size"] = 2
    ecfg["metrics"]["name"] = ["FWL", "RSAT"]
    _res, base = _driver(tmp_path, ecfg, "--render", "device", *(["--resident"] if loader == "resident" else []))
    want = _visits(2)
    assert sorted(p.name for p in base.iterdir()) == sorted(want)

    def window_image(name, k):
        xs, ys, pos = (a[k * SEQ_WINDOW:(k + 1) * SEQ_WINDOW] for a in events[name])
        cnt = np.zeros((2, H, W), np.float32)
        np.add.at(cnt, (np.where(pos, 0, 1), ys, xs), 1.0)
        return R.counts(cnt, "green_red")[0]

    for folder, (name, windows) in want.items():
        stored = sorted(p.name for p in (base / folder / "events").iterdir())
        assert stored == ["%09d.png" % k for k in range(windows)], (folder, stored)
        assert len((base / folder / "timestamps.txt").read_text().splitlines()) == windows
        for k in (0, windows - 1):
            assert np.array_equal(_read_png(base / folder / "events" / ("%09d.png" % k)), window_image(name, k)), (folder, k)
        assert {p.name for p in (base / folder / "iwe_window").iterdir()} <= set(stored)
    assert any((base / f / "iwe_window").iterdir() for f in want)
