"""Stored visualisations -- counterpart of the rendering half of reference utils/visualization.py (colour coding
:230-315, folder layout and file names of `Visualization.store` :120-226) with numpy + zlib only (the reference needs
cv2 and matplotlib).  The colour coding (flow_to_image, minmax_norm, events_to_image) is pinned by fixture G17 = the
reference's own functions run on seeded inputs (tools/make_vis_fixture.py; matplotlib exists in the image's conda
interpreter); what goes through cv2 in the reference -- resizing, BGR file writing, the live window (`update`, :28-118) --
has no counterpart to compare with here: the PNG container and the folder layout are checked structurally only.

Two renderers.  `render="host"` (the default): tensors are fetched once per stored frame and colour-coded in numpy.
`render="device"`: every image of a pass, for every sample of the batch, is colour-coded by ONE launch of evf_render_sheet
(csrc/evf_render.hip) into a uint8 frame sheet that comes back in one copy to pinned memory; only the PNG encoding (zlib)
stays on the host.  Nothing here is on the training path."""

import ctypes
import math
import os
import struct
import zlib

import numpy as np

RENDER_COUNTS, RENDER_FLOW, RENDER_FRAME = 0, 1, 2  # EVF_RENDER_* of include/evflow.h
SCHEMES = {"green_red": 0, "gray": 1}


def write_png(path, img):
    """8-bit grey [H,W] or RGB [H,W,3] PNG."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    color = 2 if img.ndim == 3 else 0
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def _hsv_to_rgb(h, s, v):
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i.astype(np.int64) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=-1)


def flow_to_image(flow_x, flow_y):
    """[H,W] x / y flow -> [H,W,3] uint8 RGB: hue = direction, value = magnitude stretched to the image's range
    (reference :230-255)."""
    mag = np.hypot(flow_x, flow_y)
    lo, span = mag.min(), mag.max() - mag.min()
    val = (mag - lo) / span if span != 0.0 else mag - lo
    hue = (np.arctan2(flow_y, flow_x) + np.pi) / (2.0 * np.pi)
    return (255 * _hsv_to_rgb(hue, np.ones_like(hue), val)).astype(np.uint8)


def minmax_norm(x):
    """Robust min-max normalisation between the 1st and 99th percentile (reference :257-267)."""
    lo, hi = np.percentile(x, 1), np.percentile(x, 99)
    if hi - lo != 0:
        x = (x - lo) / (hi - lo)
    return np.clip(x, 0, 1)


def events_to_image(event_cnt, color_scheme="green_red"):
    """[H,W,2] per-polarity counts -> [H,W] grey or [H,W,3] image in [0,1]; green_red is in the reference's channel
    order (index 1 = positive, index 2 = negative; it is written through cv2, i.e. as B,G,R) (reference :269-315)."""
    pos, neg = event_cnt[:, :, 0].astype(np.float64), event_cnt[:, :, 1].astype(np.float64)
    top = max(np.percentile(pos, 99), np.percentile(neg, 99))
    out = []
    for img in (pos, neg):
        lo = np.percentile(img, 1)
        out.append(np.clip((img - lo) / (top - lo) if lo != top else img, 0, 1))
    pos, neg = out
    if color_scheme == "gray":
        return 0.5 + 0.5 * pos - 0.5 * neg
    image = np.zeros(event_cnt.shape[:2] + (3,))
    image[:, :, 1] = pos
    image[:, :, 2] = neg
    return image


def percentile_position(n, p):
    """Where np.percentile(x, p, method="linear") of n values looks: (k, g) with the result lerp(sorted[k], sorted[min(k + 1,
    n - 1)], g).  numpy's own index arithmetic (lib/_function_base_impl.py: the `linear` entry of _QuantileMethods, _get_indexes,
    _get_gamma) in Python floats: q = p / 100, vi = (n - 1) q -- numpy's form for this method, NOT the general n q + (alpha +
    q (1 - alpha - beta)) - 1 with alpha = beta = 1, which is the same number on paper and another one in float64 (n = 2, p = 30:
    0.3 against 0.2999999999999998) --, k = floor(vi), g = vi - k.  A position at or behind the last value is (n - 1, 0.0), one
    before the first (0, 0.0), as numpy takes previous == next there."""
    q = p / 100
    vi = (n - 1) * q
    if vi >= n - 1:
        return n - 1, 0.0
    if vi < 0:
        return 0, 0.0
    k = math.floor(vi)
    return int(k), vi - k


def render_sheet(images, scheme="green_red"):
    """`images`: a list of up to eight (kind, tensor) -- RENDER_COUNTS / RENDER_FLOW with float32 [B,2,H,W], RENDER_FRAME with uint8
    [B,2,H,W], all on the current CUDA device -> the colour-coded frame sheet, a device tensor uint8 [B, nimg, H, W, 3] in PNG
    channel order, by one launch of evf_render_sheet (the count images byte-equal to events_to_image(...) * 255 -> _u8)."""
    import torch

    from .. import _lib

    if not images or len(images) > 8:
        raise _lib.EvflowError(f"render_sheet takes 1 to 8 images, not {len(images)}")
    if scheme not in SCHEMES:
        raise _lib.EvflowError(f"render_sheet: unknown colour scheme {scheme!r} (green_red, gray)")
    shape, keep = tuple(images[0][1].shape), []
    for kind, t in images:
        want = torch.uint8 if kind == RENDER_FRAME else torch.float32
        if kind not in (RENDER_COUNTS, RENDER_FLOW, RENDER_FRAME) or tuple(t.shape) != shape or len(shape) != 4 or shape[1] != 2:
            raise _lib.EvflowError(f"render_sheet: image of kind {kind} with shape {tuple(t.shape)}; every image is [B,2,H,W] like the first")
        if not t.is_cuda or t.device.index != torch.cuda.current_device():
            raise _lib.EvflowError(f"render_sheet: tensor on {t.device}; the renderer runs on the current CUDA device (no CPU fallback)")
        keep.append(t.detach().to(want).contiguous())
    B, _, H, W = shape
    n = H * W
    (k_lo, g_lo), (k_hi, g_hi) = percentile_position(n, 1), percentile_position(n, 99)
    out = torch.empty((B, len(keep), H, W, 3), dtype=torch.uint8, device=keep[0].device)
    src = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    kinds = (ctypes.c_int * len(keep))(*[k for k, _ in images])
    _lib.call("evf_render_sheet", src, kinds, len(keep), B, H, W, SCHEMES[scheme], k_lo, g_lo, k_hi, g_hi, out.data_ptr())
    return out


def _hwc(t, channels):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a.transpose(0, 2, 3, 1).reshape(a.shape[2], a.shape[3], channels)


def _u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


class Visualization:
    """`store()` of the reference (:120-226): one numbered PNG per element and call under
    <path_results>results/eval_<id>/<sequence>/{events,events_window,flow,flow_window,gtflow,frames,iwe,iwe_window}/
    plus timestamps.txt.  render="host": batch size 1, as in the reference.  render="device": any batch size, `sequence` a
    list with one folder name per slot; image counter and timestamps.txt are kept per folder."""

    FOLDERS = ("events", "events_window", "flow", "flow_window", "gtflow", "frames", "iwe", "iwe_window")
    KINDS = {"events": RENDER_COUNTS, "events_window": RENDER_COUNTS, "flow": RENDER_FLOW, "flow_window": RENDER_FLOW,
             "gtflow": RENDER_FLOW, "frames": RENDER_FRAME, "iwe": RENDER_COUNTS, "iwe_window": RENDER_COUNTS}

    def __init__(self, kwargs, eval_id=-1, path_results=None, render="host"):
        if render not in ("host", "device"):
            raise ValueError(f"Visualization(render={render!r}): host or device")
        self.render = render
        self._folders = {}   # render="device": folder -> [next image index, timestamps.txt handle or None while no slot is on it]
        self._pinned = None  # render="device": the reused pinned bytes the frame sheet is copied into
        self.img_idx = 0
        self.px = kwargs.get("vis", {}).get("px", 400)
        self.color_scheme = "green_red"
        self.store_dir = self.store_file = None
        if eval_id >= 0 and path_results is not None:
            self.store_dir = os.path.join(path_results, "results", "eval_" + str(eval_id)) + "/"
            os.makedirs(self.store_dir, exist_ok=True)

    def _events_png(self, path, cnt):
        img = events_to_image(cnt, self.color_scheme) * 255
        write_png(path, _u8(img[:, :, ::-1] if img.ndim == 3 else img))  # cv2 order B,G,R -> PNG order R,G,B

    def store(self, inputs, flow, iwe, sequence, events_window=None, masked_window_flow=None, iwe_window=None, ts=None):
        if self.store_dir is None:
            raise ValueError("Visualization(..., eval_id, path_results) is needed to store images")
        if self.render == "device":
            return self._store_device(inputs, flow, iwe, sequence, events_window, masked_window_flow, iwe_window, ts)
        path_to = self.store_dir + sequence + "/"
        if not os.path.exists(path_to):  # new sequence
            for sub in self.FOLDERS:
                os.makedirs(path_to + sub)
            if self.store_file is not None:
                self.store_file.close()
            self.store_file = open(path_to + "timestamps.txt", "w")
            self.img_idx = 0
        name = "/%09d.png" % self.img_idx
        for sub, cnt in (("events", inputs.get("event_cnt")), ("events_window", events_window), ("iwe", iwe), ("iwe_window", iwe_window)):
            if cnt is not None:
                self._events_png(path_to + sub + name, _hwc(cnt, 2))
        for sub, fl in (("flow", flow), ("flow_window", masked_window_flow), ("gtflow", inputs.get("gtflow"))):
            if fl is not None:
                f = _hwc(fl, 2)
                write_png(path_to + sub + name, flow_to_image(f[:, :, 0], f[:, :, 1]))
        if inputs.get("frames") is not None:
            write_png(path_to + "frames" + name, _u8(_hwc(inputs["frames"], 2)[:, :, 1]))
        if ts is not None:
            self.store_file.write(str(ts) + "\n")
            self.store_file.flush()
        self.img_idx += 1

    def _store_device(self, inputs, flow, iwe, sequence, events_window, masked_window_flow, iwe_window, ts):
        """One evf_render_sheet launch for every image present (in the order of FOLDERS) and every slot, one copy of the sheet into
        the reused pinned buffer, then the PNGs of slot b under folder sequence[b]."""
        import torch

        present = {"events": inputs.get("event_cnt"), "events_window": events_window, "flow": flow, "flow_window": masked_window_flow,
                   "gtflow": inputs.get("gtflow"), "frames": inputs.get("frames"), "iwe": iwe, "iwe_window": iwe_window}
        subs = [sub for sub in self.FOLDERS if present[sub] is not None]
        sequence = [sequence] if isinstance(sequence, str) else list(sequence)
        if not subs:
            raise ValueError("store(): no image to render")
        B = present[subs[0]].shape[0]
        if len(sequence) != B or len(set(sequence)) != B:
            raise ValueError(f"store(render='device'): {B} slots need {B} different folder names, got {sequence}")
        sheet = render_sheet([(self.KINDS[sub], present[sub]) for sub in subs], self.color_scheme)
        # one pinned buffer for the largest sheet of this batch shape (all eight images), allocated once: the number of images
        # changes from pass to pass (the window images come and go), the buffer's leading bytes take the sheet as it is
        most = sheet.numel() // len(subs) * len(self.FOLDERS)
        if self._pinned is None or self._pinned.numel() != most:
            self._pinned = torch.empty(most, dtype=torch.uint8, pin_memory=True)
        landed = self._pinned[:sheet.numel()].view(sheet.shape)
        landed.copy_(sheet, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        host = landed.numpy()
        ts = None if ts is None else (list(ts) if isinstance(ts, (list, tuple)) else [ts] * B)
        # a folder keeps its image counter for the life of this object; its timestamps.txt is closed while no slot stores into
        # it and reopened for appending if a slot comes back to it
        for other, state in self._folders.items():
            if other not in sequence and state[1] is not None:
                state[1].close()
                state[1] = None
        for b, folder in enumerate(sequence):
            path_to = self.store_dir + folder + "/"
            if folder not in self._folders:  # new sequence in this slot
                for sub in self.FOLDERS:
                    os.makedirs(path_to + sub, exist_ok=True)
                self._folders[folder] = [0, open(path_to + "timestamps.txt", "w")]
            state = self._folders[folder]
            if state[1] is None:
                state[1] = open(path_to + "timestamps.txt", "a")
            name = "/%09d.png" % state[0]
            for k, sub in enumerate(subs):
                write_png(path_to + sub + name, host[b, k, :, :, 0] if sub == "frames" else host[b, k])
            if ts is not None:
                state[1].write(str(ts[b]) + "\n")
                state[1].flush()
            state[0] += 1
