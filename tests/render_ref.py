"""The float64 numpy restatement of evf_render_sheet's three image kinds (csrc/evf_render.hip, contract in include/evflow.h) and
the seeded inputs shared by tests/test_host_render_reference.py (which pins this file to utils/visualization.py and to fixture
G17 without a device) and tests/test_gpu_render.py.  Not a test module.

Every function returns (u8, pre): the uint8 image [H,W,3] in PNG channel order and the float64 value of every channel before
the quantisation (255 c), which the flow rule of the GPU test needs."""

import functools
import os

import numpy as np

from event_flow_amd.utils.visualization import percentile_position

F32, F64 = np.float32, np.float64
COUNTS, FLOW, FRAME = 0, 1, 2
SCHEMES = ("green_red", "gray")
#          n = 2   6       35      256       > one stride of the block, odd   a DAVIS240 frame
SHAPES = [(1, 2), (2, 3), (5, 7), (16, 16), (33, 65), (180, 240)]
COUNT_CONTENTS = ("zero", "single", "const3", "poisson", "distinct", "fractional")
FLOW_CONTENTS = ("normal", "axis", "zero", "const", "signed_zero")


def lerp(a, b, g):
    """numpy's _lerp for scalars, float64."""
    a, b, g = F64(a), F64(b), F64(g)
    d = b - a
    return b - d * (F64(1.0) - g) if g >= 0.5 else a + d * g


def percentile(x, p):
    """np.percentile(x, p) from the order statistics: sorted[k], sorted[min(k + 1, n - 1)] and the lerp."""
    s = np.sort(np.asarray(x, F64).ravel())
    k, g = percentile_position(s.size, p)
    return lerp(s[k], s[min(k + 1, s.size - 1)], g)


def counts(x, scheme):
    """x float32 [2,H,W] (positive, negative) -> events_to_image(...) * 255 -> rint -> clip."""
    x = np.asarray(x, F32).astype(F64)
    top = max(percentile(x[0], 99), percentile(x[1], 99))
    c01 = []
    for c in range(2):
        lo = percentile(x[c], 1)
        c01.append(np.clip((x[c] - lo) / (top - lo) if lo != top else x[c], 0.0, 1.0))
    pos, neg = c01
    if scheme == "gray":
        g = (0.5 + 0.5 * pos - 0.5 * neg) * 255.0
        pre = np.stack([g, g, g], -1)
    else:
        pre = np.stack([neg * 255.0, pos * 255.0, np.zeros_like(pos)], -1)
    return np.clip(np.rint(pre), 0, 255).astype(np.uint8), pre


def flow(f):
    """f float32 [2,H,W] (x, y) -> flow_to_image in float64."""
    fx, fy = np.asarray(f, F32).astype(F64)
    mag = np.hypot(fx, fy)
    lo, span = mag.min(), mag.max() - mag.min()
    val = (mag - lo) / span if span != 0.0 else mag - lo
    hue = (np.arctan2(fy, fx) + np.pi) / (2.0 * np.pi)
    h6 = hue * 6.0
    i = np.floor(h6)
    fr = h6 - i
    p, q, t = val * (1.0 - 1.0), val * (1.0 - 1.0 * fr), val * (1.0 - 1.0 * (1.0 - fr))
    i = i.astype(np.int64) % 6
    r = np.choose(i, [val, q, p, p, t, val])
    g = np.choose(i, [t, val, val, q, p, p])
    b = np.choose(i, [p, p, t, val, val, q])
    pre = 255.0 * np.stack([r, g, b], -1)
    return pre.astype(np.uint8), pre


def frame(f):
    """f uint8 [2,H,W] -> channel 1 in R = G = B."""
    g = np.asarray(f, np.uint8)[1]
    return np.stack([g, g, g], -1), np.stack([g, g, g], -1).astype(F64)


KIND_FN = {FLOW: flow, FRAME: frame}


def _rng(*key):
    return np.random.default_rng([17] + [int(k) for k in key])


def count_image(content, H, W, seed):
    """One float32 [2,H,W] count image."""
    r, n = _rng(1, COUNT_CONTENTS.index(content), H, W, seed), H * W
    if content == "zero":
        x = np.zeros((2, H, W))
    elif content == "single":  # one polarity only (the other all zero)
        x = np.stack([r.poisson(1.5, (H, W)), np.zeros((H, W))])
    elif content == "const3":  # lo == top
        x = np.full((2, H, W), 3.0)
    elif content == "poisson":  # heavy ties
        x = r.poisson(0.3, (2, H, W)).astype(F64)
    elif content == "distinct":  # every order statistic differs from the next one
        x = np.stack([r.permutation(n) * 0.37 + 0.11, r.permutation(n) * 1.3 - 0.4 * n]).reshape(2, H, W)
    else:  # fractional and negative values: an IWE without rounding
        x = r.normal(0.4, 1.7, (2, H, W))
    return np.ascontiguousarray(x, F32)


def flow_image(content, H, W, seed):
    """One float32 [2,H,W] flow map."""
    r = _rng(2, FLOW_CONTENTS.index(content), H, W, seed)
    if content == "normal":  # (span >= 1 from 4 pixels on; asserted by the host test)
        f = r.normal(0.0, 3.0, (2, H, W))
    elif content == "axis":  # along the axes, both signs, and a few zeros
        m = r.integers(0, 5, (H, W))
        a = r.uniform(0.5, 4.0, (H, W))
        f = np.stack([np.where(m == 0, a, np.where(m == 1, -a, 0.0)), np.where(m == 2, a, np.where(m == 3, -a, 0.0))])
    elif content == "zero":
        f = np.zeros((2, H, W))
    elif content == "const":  # span == 0 with a magnitude
        f = np.stack([np.full((H, W), 1.25), np.full((H, W), -0.75)])
    else:  # +0.0 / -0.0 components beside ordinary ones
        f = r.normal(0.0, 2.0, (2, H, W))
        z = r.integers(0, 4, (2, H, W))
        f = np.where(z == 0, 0.0, np.where(z == 1, -0.0, f))
    return np.ascontiguousarray(f, F32)


def frame_image(H, W, seed):
    return _rng(3, H, W, seed).integers(0, 256, (2, H, W)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def count_batch(content, H, W, B):
    """[B,2,H,W]: sample b holds content number (index + b) with seed b -- different content per sample."""
    j = COUNT_CONTENTS.index(content)
    x = np.stack([count_image(COUNT_CONTENTS[(j + b) % len(COUNT_CONTENTS)], H, W, b) for b in range(B)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def count_ref(content, H, W, B, scheme):
    """The restatement of count_batch(...): (u8 [B,H,W,3], pre [B,H,W,3]), computed once and read-only."""
    out = [counts(x, scheme) for x in count_batch(content, H, W, B)]
    u8, pre = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    u8.setflags(write=False)
    pre.setflags(write=False)
    return u8, pre


def g17():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_visualization.npz"))


@functools.lru_cache(maxsize=None)
def flow_inputs():
    """name -> float32 [B,2,H,W]: the G17 flow inputs (one batch of four) and every seeded content at two shapes, B = 1 and 3."""
    g = g17()
    out = {"g17": np.stack([np.stack([g[f"flow{k}_x"], g[f"flow{k}_y"]]) for k in range(4)]).astype(F32)}
    for content in FLOW_CONTENTS:
        out[content + "_1"] = np.stack([flow_image(content, 33, 65, 0)])
        out[content + "_3"] = np.stack([flow_image(FLOW_CONTENTS[(FLOW_CONTENTS.index(content) + b) % len(FLOW_CONTENTS)], 16, 24, b)
                                        for b in range(3)])
    out["normal_davis"] = np.stack([flow_image("normal", 180, 240, 7)])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def flow_ref(name):
    out = [flow(f) for f in flow_inputs()[name]]
    u8, pre = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    u8.setflags(write=False)
    pre.setflags(write=False)
    return u8, pre


def g17_bar(got, ref):
    """The project's bar of fixture G17 (tests/test_host_visualization.py): no channel off by more than one level, fewer than 1 %
    of the values off at all.  -> (largest difference, share of values that differ)."""
    d = np.abs(np.asarray(got).astype(int) - np.asarray(ref).astype(int))
    return int(d.max()), float((d > 0).mean())
