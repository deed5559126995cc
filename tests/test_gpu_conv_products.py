"""The general-path convolutions through the C ABI against the float64 references of tests/conv_ref.py, per product:
evf_conv2d_fwd_b3 / evf_conv2d_dgrad_b3 through every member the dispatcher (b3_launch, csrc/evf_conv_b3gen.hip) can be made to take,
the fp32 kernels evf_conv2d_fwd / evf_conv2d_dgrad, evf_conv2d_fwd_b3_parts, evf_conv2d_wgrad through its bf16, fp32, promise,
four-channel, 1x1 and larger-kernel routes, and the weight packers.

IMPULSE leg (the decisive one): inputs that are zero except for isolated impulses, so that every output element is one product or
nothing.  An element with a product is held to K * 2^-24 * |x w| (K_IMP on the bf16 matrix cores, K_F32 = 1 on the fp32 kernels).  With
a base and / or bias the bf16 routes add the magnitudes, K_IMP * 2^-24 * (|base| + |bias| + |x w|).  The fp32 kernels stay at K = 1,
but one unit of |base| + |bias| + |x w| is not what correct fp32 arithmetic gives -- (fl(x w) + bias) + old rounds three times -- so
their accumulate sub-cases are held to one unit PER ROUNDING of the magnitude it rounds: 2^-24 * (|x w| + |x w + bias| + |x w + bias +
old|), tighter than three units of the summed magnitudes.  An element without a product must have the exact bits of 0, the base or the bias.  This is what fails when a
member drops one of the six split terms.
DENSE leg: random operands, every element within K_SUM * 2^-24 * A_e of float64, A_e the float64 product of the absolute values
(+ |bias| + |base|).  It need not reject a dropped third-order term (2^-16 of one product is below the rounding of a sum of hundreds):
that is the impulse leg's job; it rejects wrong taps, borders, channel tails and a weight gradient that rounded a real value to bf16.

Every operand sits between guard regions (gpu_bufs.Bufs), pixel strides wider than the channel count carry the sentinel in their
padding (unchanged in outputs, never leaking from inputs), and the bounds are established on the CPU by tests/test_host_conv_reference.py.

EVF_CONV_REPORT=<file>: per route the largest observed error as a fraction of its bound and the number of elements checked."""

import ctypes
import os

import numpy as np
import pytest
import torch

import conv_ref as R
from event_flow_amd import _lib
from gpu_bufs import SENTINEL, Bufs

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FILL = 7.0  # initial contents of outputs that a kernel must overwrite
CHAIN_SLACK = 2.0 ** -20  # second-order terms of a chain of three roundings (each magnitude is taken from the exact value)

REPORT = {}  # (leg, route) -> [worst fraction of the bound, elements checked, elements that must be exact, worst error in units]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("EVF_CONV_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write(f"bounds: K_IMP {R.K_IMP}  K_F32 {R.K_F32} (accumulating: one unit per rounding)  K_SUM {R.K_SUM}; units of 2^-24 * scale\n")
            for leg in ("impulse", "dense"):
                rows = {k[1]: v for k, v in REPORT.items() if k[0] == leg}
                if rows:
                    f.write(f"{leg} leg: {len(rows)} routes, worst error / bound {max(v[0] for v in rows.values()):.3f}, "
                            f"{sum(v[1] for v in rows.values())} elements within bounds, {sum(v[2] for v in rows.values())} bit-exact\n")
                if leg == "impulse":  # the split products on the bf16 matrix cores alone: what K_IMP was derived for
                    split = [v[3] for r, v in rows.items() if "fp32" not in r and "wgrad" not in r or "bf16" in r or "promise" in r]
                    f.write(f"impulse leg, split products on the bf16 matrix cores: largest observed error {max(split):.2f} units of "
                            f"2^-24 |x w| over {len(split)} routes (K_IMP {R.K_IMP})\n")
                for route, v in sorted(rows.items()):
                    f.write(f"  {leg} {route}: error / bound {v[0]:.3f} ({v[3]:.2f} units)  elements {v[1]}  bit-exact {v[2]}\n")


@pytest.fixture(autouse=True)
def _defaults():
    yield
    L = _lib.load()
    L.evf_conv_tile_select(-1)
    L.evf_conv_split_select(0)
    L.evf_wgrad_teams_select(0)


def note(leg, route, frac, n, nexact=0, units=0.0):
    r = REPORT.setdefault((leg, route), [0.0, 0, 0, 0.0])
    r[0] = max(r[0], float(frac))
    r[3] = max(r[3], float(units))
    r[1] += int(n)
    r[2] += int(nexact)


def P(b):
    return None if b is None else b.ptr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def within(leg, route, what, got, ref, scale, k, mask=None):
    """|got - ref| <= k * 2^-24 * scale on every (masked) element; prints and records the fraction of the bound that was used."""
    got, ref, scale = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(scale, F64)
    assert np.isfinite(got).all(), f"{route} {what}: non-finite output"
    if mask is not None:
        got, ref, scale = got[mask], ref[mask], scale[mask]
    u = R.dense_units(got.reshape(-1), ref.reshape(-1), scale.reshape(-1)) / k
    i = int(np.argmax(u)) if u.size else 0
    worst = float(u[i]) if u.size else 0.0
    print(f"  {leg} {route} {what}: {worst:.3f} of the bound over {u.size} elements")
    note(leg, route, worst, u.size, units=worst * k)
    assert worst <= 1.0, (f"{route} {what}: error {abs(got.reshape(-1)[i] - ref.reshape(-1)[i]):.4g} = {worst * k:.2f} units > {k} at {i} "
                          f"(got {got.reshape(-1)[i]!r}, ref {ref.reshape(-1)[i]!r}); {int((u > 1).sum())} of {u.size} violate")


def padded(a, ld):
    """[..., C] -> [..., ld] with the sentinel in the padding floats of every pixel."""
    out = np.full(a.shape[:-1] + (ld,), SENTINEL, F32)
    out[..., :a.shape[-1]] = a
    return out


def unpad(buf, C):
    """Payload of a padded output; its padding must still hold the sentinel."""
    a = buf.get()
    assert (a[..., C:] == SENTINEL).all(), "a kernel wrote into the padding floats of a pixel"
    return a[..., :C]


# ================================================================================================================ packing
def pack(B, w, transpose, b3, cin_total=None, cin_off=0, Cin=None):
    """evf_pack_conv2d_weight[_b3] into a guarded buffer of exactly the packed size, pre-filled with the sentinel."""
    L = _lib.load()
    Cout, ct, k, _ = w.shape
    Cin = ct if Cin is None else Cin
    n = (L.evf_conv2d_b3_packed_size if b3 else L.evf_conv2d_packed_size)(Cout, Cin, k, transpose)
    assert n > 0
    dst = B.new(np.full(n, SENTINEL, F32))
    src = B.new(w)
    _lib.call("evf_pack_conv2d_weight_b3" if b3 else "evf_pack_conv2d_weight", src.ptr, Cout, Cin, k, transpose, ct if cin_total is None else cin_total,
              cin_off, dst.ptr)
    return dst


PACK_TENSORS = [(40, 66, 3, 0, 74, 4), (36, 20, 5, 1, 20, 0), (5, 130, 1, 0, 130, 0), (132, 32, 3, 1, 40, 8)]  # Cout, Cin, k, transpose, cin_total, cin_off


def test_pack_kernels_fill_exactly_their_packed_size():
    """evf_conv2d_packed_size / evf_conv2d_b3_packed_size size the guarded buffers: the pack kernels leave no sentinel inside (they
    write every float, padding included) and the guards stay intact."""
    B = Bufs()
    rng = np.random.default_rng(1)
    for Cout, Cin, k, tr, ct, off in PACK_TENSORS:
        w = R.weights(rng, (Cout, ct, k, k))
        for b3 in (True, False):
            got = pack(B, w, tr, b3, ct, off, Cin).get()
            assert not (got == SENTINEL).any() and np.isfinite(got).all(), (Cout, Cin, k, tr, b3)
            inside = w[:, off:off + Cin].astype(F64)
            if b3:  # a checksum only: the bf16 pairs of the three planes add up to the weights of the packed range (the layout itself is held by the conv tests)
                h = got.view(np.uint32)
                total = (h << 16).view(F32).astype(F64).sum() + (h & 0xFFFF0000).view(F32).astype(F64).sum()
            else:
                total = got.astype(F64).sum()
            assert abs(total - inside.sum()) <= 1e-9 * np.abs(inside).sum(), (Cout, Cin, k, tr, b3)
    B.check()


def test_pack_multi_is_byte_identical_to_one_call_per_tensor():
    B = Bufs()
    L = _lib.load()
    rng = np.random.default_rng(2)
    srcs, single, multi, meta = [], [], [], []
    for Cout, Cin, k, tr, ct, off in PACK_TENSORS:
        w = R.weights(rng, (Cout, ct, k, k))
        srcs.append(B.new(w))
        single.append(pack(B, w, tr, True, ct, off, Cin))
        multi.append(B.new(np.full(L.evf_conv2d_b3_packed_size(Cout, Cin, k, tr), SENTINEL, F32)))
        meta += [Cout, Cin, k, tr, ct, off]
    n = len(srcs)
    _lib.call("evf_pack_conv2d_weights_b3_multi", (ctypes.c_void_p * n)(*[s.ptr for s in srcs]), (ctypes.c_void_p * n)(*[m.ptr for m in multi]),
              (ctypes.c_int * len(meta))(*meta), n)
    for s, m, t in zip(single, multi, PACK_TENSORS):
        assert same_bits(s.get(), m.get()), t
    B.check()


# ================================================================================================== forward / input gradient
class Conv:
    """One (shape, direction, entry point) with its packed weights and scratch; launches on guarded operands."""

    def __init__(self, B, shape, direction, b3, rng, flags=0):
        self.B, self.shape, self.dir, self.b3, self.flags = B, shape, direction, b3, flags
        Bn, Cin, Cout, H, W, k, s = shape
        self.fwd = direction == "fwd"
        OH, OW = R.out_dim(H, k, s), R.out_dim(W, k, s)
        self.K, self.N = (Cin, Cout) if self.fwd else (Cout, Cin)
        self.src_shape = (Bn, H, W, Cin) if self.fwd else (Bn, OH, OW, Cout)
        self.out_shape = (Bn, OH, OW, Cout) if self.fwd else (Bn, H, W, Cin)
        self.w_wide = R.weights(rng, (Cout, Cin + 8, k, k))  # the layer's weight inside a wider tensor (cin_total = Cin + 8, cin_off = 4)
        self.w = np.ascontiguousarray(self.w_wide[:, 4:4 + Cin])
        tr = 0 if self.fwd else 1
        self.wp = pack(B, self.w, tr, b3)
        self.wp_wide = pack(B, self.w_wide, tr, b3, Cin + 8, 4, Cin)
        self.ws, self.nws = None, 0
        if b3:
            self.nws = int(_lib.load().evf_conv2d_b3_ws(*self.out_shape))
            if self.nws > 0:
                self.ws = B.new(np.full(self.nws, SENTINEL, F32))

    def run(self, src, out_init, *, bias=None, acc=0, ld_pad=0, wide=False):
        """-> output payload.  src / out_init: dense arrays; ld_pad > 0 puts both into pixel strides C + ld_pad."""
        Bn, Cin, Cout, H, W, k, s = self.shape
        lds, ldo = self.K + ld_pad, self.N + ld_pad
        sb = self.B.new(padded(src, lds))
        ob = self.B.new(padded(out_init, ldo))
        bb = self.B.new(bias) if bias is not None else None
        wp = self.wp_wide if wide else self.wp
        ldx, ldy = (lds, ldo) if self.fwd else (ldo, lds)
        fl = acc | self.flags
        if self.b3 and self.fwd:
            _lib.call("evf_conv2d_fwd_b3", sb.ptr, ldx, wp.ptr, P(bb), ob.ptr, ldy, Bn, H, W, Cin, Cout, k, s, fl, P(self.ws), self.nws)
        elif self.b3:
            _lib.call("evf_conv2d_dgrad_b3", sb.ptr, ldy, wp.ptr, ob.ptr, ldx, Bn, H, W, Cin, Cout, k, s, fl, P(self.ws), self.nws)
        elif self.fwd:
            _lib.call("evf_conv2d_fwd", sb.ptr, ldx, wp.ptr, P(bb), ob.ptr, ldy, Bn, H, W, Cin, Cout, k, s, fl)
        else:
            _lib.call("evf_conv2d_dgrad", sb.ptr, ldy, wp.ptr, ob.ptr, ldx, Bn, H, W, Cin, Cout, k, s, fl)
        torch.cuda.synchronize()
        return unpad(ob, self.N)


def check_impulse(route, what, got, case, k, base=None, bias=None, chain=False):
    """One impulse launch: elements with a product within k * 2^-24 * (|x w| + |base| + |bias|) -- chain (fp32 kernels): within
    k * 2^-24 * (|x w| + |x w + bias| + |x w + bias + base|), one unit per correctly rounded operation --, all others bit-exact."""
    hit = case["hit"]
    scale = np.abs(case["ref"])
    want = case["ref"].copy()
    exact = np.zeros(hit.shape, F32)  # what (0 + bias) + base gives in fp32 where there is no product
    for extra in (bias, base):
        if extra is not None:
            e = np.broadcast_to(np.asarray(extra, F32), hit.shape)
            want = want + e.astype(F64)
            scale = scale + (np.abs(want) if chain else np.abs(e.astype(F64)))
            exact = (exact + e).astype(F32)
    within("impulse", route, what, got, want, scale * (1 + CHAIN_SLACK if chain else 1), k, mask=hit)
    nothing = ~hit
    note("impulse", route, 0.0, 0, int(nothing.sum()))
    assert same_bits(got[nothing], exact[nothing]), (f"{route} {what}: {int((got[nothing] != exact[nothing]).sum())} elements without a product "
                                                     f"differ from the exact value (first {got[nothing][got[nothing] != exact[nothing]][:3]})")


def impulse_route(route, shape, direction, b3, ld_pad, flags=0, exact_from=None):
    """All impulse launches of one route: both lattice phases x the rounds that reach every contraction channel, overwriting a
    buffer pre-filled with 7; then on the operands of phase 1 / round 0: accumulate into a randn base (with a bias on the forward),
    pixel strides wider than the channel counts, and the weights packed out of a wider tensor."""
    B = Bufs()
    rng = np.random.default_rng(abs(hash(shape)) % 2 ** 31)
    c = Conv(B, shape, direction, b3, rng, flags)
    assert same_bits(c.wp.get(), c.wp_wide.get()), "packing a channel range of a wider weight differs from packing the range alone"
    k = R.K_IMP if b3 else R.K_F32
    fill = np.full(c.out_shape, FILL, F32)
    last = None
    for phase in (0, 1):
        for rnd in range(R.impulse_rounds(shape, direction)):
            case = R.impulse_case(shape, direction, phase, rnd, c.w, exact_from=exact_from)
            check_impulse(route, f"phase {phase} round {rnd}", c.run(case["src"], fill), case, k)
            if rnd == 0:
                last = case
    base = rng.standard_normal(c.out_shape).astype(F32)
    bias = rng.standard_normal(c.N).astype(F32) if c.fwd else None
    check_impulse(route, "accumulate", c.run(last["src"], base, bias=bias, acc=1), last, k, base=base, bias=bias, chain=not b3)
    check_impulse(route, f"ld + {ld_pad}", c.run(last["src"], fill, ld_pad=ld_pad), last, k)
    check_impulse(route, "wide weight", c.run(last["src"], fill, wide=True), last, k)
    B.check()
    return c, last


def select(monkeypatch, tile, split=0, nstream=False):
    """Force the dispatcher: evf_conv_tile_select / evf_conv_split_select (restored by the _defaults fixture) and EVF_CONV_NSTREAM,
    which b3_launch reads at every call (restored by monkeypatch)."""
    monkeypatch.setenv("EVF_CONV_NSTREAM", "2" if nstream else "1")
    L = _lib.load()
    assert L.evf_conv_tile_select(tile) == 0 and L.evf_conv_split_select(split) == 0


GEN_SHAPES = [(1, 4, 8, 9, 7, 3, 1), (2, 66, 16, 10, 13, 3, 1), (3, 5, 7, 11, 13, 3, 2), (1, 20, 36, 10, 13, 3, 2), (1, 6, 8, 13, 10, 5, 1),
              (1, 16, 16, 15, 15, 7, 2), (1, 32, 3, 17, 33, 1, 1), (1, 30, 2, 17, 33, 1, 1)]
TILE_SHAPES = [(2, 132, 64, 17, 33, 3, 1), (1, 32, 132, 17, 33, 3, 1), (1, 20, 96, 18, 34, 3, 1)]
IMG_SHAPES = [(2, 128, 192, 16, 16, 3, 1), (1, 96, 64, 13, 16, 3, 1), (3, 64, 40, 4, 7, 3, 1)]
NSTREAM_KN = [(2, 32, 132, 9, 33), (1, 64, 260, 9, 33)]  # B, K contraction channels, N output channels, H, W


def sid(shape):
    return "x".join(str(v) for v in shape)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", GEN_SHAPES, ids=sid)
def test_impulse_general_b3_kernel(shape, direction, monkeypatch):
    """evf_conv_tile_select(0): b3_launch skips the 3x3 family and takes k_conv2d_b3 (csrc/evf_conv_b3gen.hip) -- VEC 4 / 2 / 1 by
    channel count and pixel stride (the ld + 3 sub-case is the scalar loader), the transposed epilogue where ldo % 32 == 0, and for
    the input gradient of a 3x3 stride-2 product its parity form (PAR: 20 -> 36 channels at stride 2 and 5 -> 7)."""
    select(monkeypatch, 0)
    impulse_route(f"general b3 {direction}", shape, direction, True, 3)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", GEN_SHAPES, ids=sid)
def test_impulse_fp32_kernels(shape, direction):
    """evf_conv2d_fwd / evf_conv2d_dgrad (k_conv2d_f32, csrc/evf_conv_gen.hip): one correctly rounded product, K = 1; accumulating,
    one unit per rounding of (fl(x w) + bias) + old (module docstring)."""
    impulse_route(f"fp32 {direction}", shape, direction, False, 3)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=sid)
def test_impulse_tile_kernel(shape, direction, monkeypatch):
    """evf_conv_tile_select(2), images larger than 16 x 16, EVF_CONV_NSTREAM != 2: evf_conv3_b3i_plan refuses (H, W > I_DIM), the
    N-streaming member is not forced and its own plan refuses (< 160 blocks), evf_conv3_b3t_plan (force) takes the product:
    k_conv3_b3t, one row and one column past a 16 x 32 tile, the 2 x 64 + 32 tail launch (N = 132), a ragged last channel group."""
    select(monkeypatch, 2)
    impulse_route(f"tile {direction}", shape, direction, True, 4)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("kn", NSTREAM_KN, ids=sid)
def test_impulse_nstream_kernel(kn, direction, monkeypatch):
    """evf_conv_tile_select(2) with EVF_CONV_NSTREAM=2: evf_conv3_b3n_plan (force) takes the product ahead of the tile kernel:
    k_conv3_b3n, five N tiles with a 4-channel remainder on ragged 8 x 32 tiles; nine N tiles in two chunks."""
    Bn, K, N, H, W = kn
    shape = (Bn, K, N, H, W, 3, 1) if direction == "fwd" else (Bn, N, K, H, W, 3, 1)
    select(monkeypatch, 2, nstream=True)
    impulse_route(f"n-stream {direction}", shape, direction, True, 4)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", IMG_SHAPES, ids=sid)
def test_impulse_whole_image_kernel(shape, direction, monkeypatch):
    """evf_conv_tile_select(2), images of at most 16 x 16: evf_conv3_b3i_plan (force) is offered the product first: k_conv3_b3i."""
    select(monkeypatch, 2)
    impulse_route(f"whole-image {direction}", shape, direction, True, 4)


SPLIT_ROUTES = [("general b3 split", (1, 16, 16, 15, 15, 7, 2), 0, False), ("tile split", (1, 20, 96, 18, 34, 3, 1), 2, False),
                ("n-stream split", (1, 64, 260, 9, 33, 3, 1), 2, True), ("whole-image split", (1, 96, 64, 13, 16, 3, 1), 2, False)]


@pytest.mark.parametrize("route,shape,tile,nstream", SPLIT_ROUTES, ids=[r[0].replace(" ", "-") for r in SPLIT_ROUTES])
def test_impulse_forced_k_split_and_parts(route, shape, tile, nstream, monkeypatch):
    """evf_conv_split_select(3) with scratch from evf_conv2d_b3_ws: every member writes its K ranges into slabs and k_b3_reduce adds
    them in index order (the general kernel needs N % 4 == 0 for its slabs, so its shape is 16 -> 16 channels; the tile family's
    b3_plan_splits gives min(3, K / 16 chunks): 2 slabs for K = 20).  evf_conv2d_fwd_b3_parts on the same operands leaves the slabs to the caller: each holds the product or an exact 0, exactly one slab per product, and the
    slabs added in index order in fp32 are the bits evf_conv2d_fwd_b3 returns."""
    select(monkeypatch, tile, 3, nstream)
    for direction in ("fwd", "dgrad"):
        impulse_route(f"{route} {direction}", shape, direction, True, 4 if tile else 3)
    B = Bufs()
    Bn, Cin, Cout, H, W, k, s = shape
    rng = np.random.default_rng(5)
    c = Conv(B, shape, "fwd", True, rng)
    case = R.impulse_case(shape, "fwd", 1, 0, c.w)
    whole = c.run(case["src"], np.full(c.out_shape, FILL, F32))
    xb, yb = B.new(case["src"]), B.new(np.full(c.out_shape, FILL, F32))
    nparts = ctypes.c_int(-1)
    c.ws.set(np.full(c.nws, SENTINEL, F32))
    _lib.call("evf_conv2d_fwd_b3_parts", xb.ptr, Cin, c.wp.ptr, yb.ptr, Cout, Bn, H, W, Cin, Cout, k, s, 0, c.ws.ptr, c.nws, ctypes.byref(nparts))
    torch.cuda.synchronize()
    n = nparts.value
    assert n >= 2, n
    M = Bn * c.out_shape[1] * c.out_shape[2]
    slabs = c.ws.get()[:n * M * Cout].reshape((n,) + c.out_shape)
    assert same_bits(yb.get(), np.full(c.out_shape, FILL, F32))  # (in parts: y itself is not written)
    total = slabs[0].copy()
    for z in range(1, n):
        total = (total + slabs[z]).astype(F32)
    assert same_bits(total, whole)
    nonzero = slabs != 0
    assert (nonzero.sum(0) == case["hit"]).all()  # one slab holds the product, the others (and every element without one) exact zeros
    within("impulse", f"{route} parts", "slabs", slabs.sum(0, dtype=F64), case["ref"], np.abs(case["ref"]), R.K_IMP, mask=case["hit"])
    B.check()


@pytest.mark.parametrize("shape,ef", [((8, 256, 512, 16, 16, 3, 1), 0), ((2, 132, 32, 80, 130, 3, 1), 4)], ids=["two-images-per-block", "tiles-behind-a-head"])
def test_impulse_promise_route(shape, ef, monkeypatch):
    """accumulate bit 2 with exact_from: sx_plan (csrc/evf_conv_b3small.hip) accepts (8,256,512,16,16) as GEOM 0 (two 16 x 16 images
    per block, 32 blocks x 4 K splits >= 96) and (2,132,32,80,130) as GEOM 1 with a real-valued head (50 blocks x 2 splits >= 96):
    k_conv3_b3x into slabs + k_b3_reduce.  Full values only in channels below exact_from."""
    select(monkeypatch, -1)
    impulse_route("promise fwd", shape, "fwd", True, 4, flags=4 | (ef << 4), exact_from=ef)


# ================================================================================================================ weight gradient
def wgrad_call(B, case, shape, *, flags, gw_init, gb_init=None, cin_total=None, cin_off=0, ld_pad=0, ws="plan", ldx=None, x_full=None):
    Bn, Cin, Cout, H, W, k, s = shape
    L = _lib.load()
    x = case["x"] if x_full is None else x_full
    ldx = (Cin + ld_pad) if ldx is None else ldx
    xb, gb = B.new(padded(x, ldx)), B.new(padded(case["gy"], Cout + ld_pad))
    wb = B.new(gw_init)
    bb = B.new(gb_init) if gb_init is not None else None
    nws = int(L.evf_conv2d_wgrad_ws(Bn, H, W, Cin, Cout, k, s))
    wsb = B.new(np.full(max(nws, 1), SENTINEL, F32)) if (ws == "plan" and nws > 0) else None
    assert wsb is not None or k != 3
    _lib.call("evf_conv2d_wgrad", xb.ptr, ldx, gb.ptr, Cout + ld_pad, wb.ptr, P(bb), Bn, H, W, Cin, Cout, k, s, Cin if cin_total is None else cin_total,
              cin_off, flags, P(wsb))
    torch.cuda.synchronize()
    return wb.get(), (bb.get() if bb is not None else None)


def wgrad_nsplit(shape):
    Bn, Cin, Cout, H, W, k, s = shape
    return max(int(_lib.load().evf_conv2d_wgrad_ws(Bn, H, W, Cin, Cout, k, s)) // (9 * Cin * Cout), 1) if k == 3 else 1


def check_wgrad(leg, route, what, got, ref, scale, k, hit, base=None, cin_off=0, Cin=None, chain=False):
    """g_w within k * 2^-24 * (scale + |base|) -- chain (fp32 kernels accumulating): k * 2^-24 * (|x g| + |x g + base|), one unit per
    rounding --, elements without a product exact, columns outside the call's channel range untouched."""
    Cin = ref.shape[1] if Cin is None else Cin
    inside = got[:, cin_off:cin_off + Cin]
    b = None if base is None else base[:, cin_off:cin_off + Cin]
    want = ref if b is None else ref + b.astype(F64)
    sc = scale if b is None else (scale + np.abs(want)) * (1 + CHAIN_SLACK) if chain else scale + np.abs(b.astype(F64))
    within(leg, route, what, inside, want, sc, k, mask=hit)
    nothing = ~hit
    if nothing.any():
        exact = np.zeros(ref.shape, F32) if b is None else b
        note(leg, route, 0.0, 0, int(nothing.sum()))
        assert same_bits(inside[nothing], exact[nothing]), f"{route} {what}: elements without a product are not exact"
    if base is not None:  # the columns outside the call's channel range: bit-identical to the base
        assert same_bits(got[:, :cin_off], base[:, :cin_off]) and same_bits(got[:, cin_off + Cin:], base[:, cin_off + Cin:]), (route, what)


def wgrad_impulse_route(route, shape, flags, k_bound, f32, kinds="mixed", ld_pad=4, teams=0, ws="plan", bias=True):
    """Overwrite into 7 (bias gradient included), accumulate into a randn base, accumulate into a wider weight (cin_total = Cin + 8,
    cin_off = 4), and pixel strides wider than the channel counts -- one launch each on the same operands."""
    Bn, Cin, Cout, H, W, k, s = shape
    assert _lib.load().evf_wgrad_teams_select(teams) == 0
    B = Bufs()
    rng = np.random.default_rng(Cin * 1000 + Cout)
    case = R.wgrad_case(shape, wgrad_nsplit(shape), kinds=kinds)
    ref, hit, mag = case["ref"], case["hit"], np.abs(case["ref"])
    fill = np.full(ref.shape, FILL, F32)
    got, gb = wgrad_call(B, case, shape, flags=flags, gw_init=fill, gb_init=np.full(Cout, FILL, F32) if bias else None, ws=ws)
    check_wgrad("impulse", route, "overwrite", got, ref, mag, k_bound, hit)
    if bias:
        within("dense", route + " bias gradient", "overwrite", gb, case["bias_ref"], case["bias_abs"], R.K_SUM)
    base = rng.standard_normal(ref.shape).astype(F32)
    bbase = rng.standard_normal(Cout).astype(F32)
    got, gb = wgrad_call(B, case, shape, flags=flags | 1, gw_init=base, gb_init=bbase if bias else None, ws=ws)
    check_wgrad("impulse", route, "accumulate", got, ref, mag, k_bound, hit, base=base, chain=f32)
    if bias:
        within("dense", route + " bias gradient", "accumulate", gb, case["bias_ref"] + bbase, case["bias_abs"] + np.abs(bbase), R.K_SUM)
    wide = rng.standard_normal((Cout, Cin + 8, k, k)).astype(F32)
    got, _ = wgrad_call(B, case, shape, flags=flags | 1, gw_init=wide, cin_total=Cin + 8, cin_off=4, ws=ws)
    check_wgrad("impulse", route, "wide weight", got, ref, mag, k_bound, hit, base=wide, cin_off=4, Cin=Cin, chain=f32)
    got, _ = wgrad_call(B, case, shape, flags=flags, gw_init=fill, ld_pad=ld_pad, ws=ws)
    check_wgrad("impulse", route, f"ld + {ld_pad}", got, ref, mag, k_bound, hit)
    B.check()


# (the last shape is beyond the issue's four: three redo tiles, an exact one on either side of the flagged one)
WG3_SHAPES = [(2, 36, 32, 17, 23, 3, 1), (2, 72, 100, 17, 23, 3, 1), (1, 64, 128, 9, 130, 3, 1), (2, 32, 64, 12, 12, 3, 2), (2, 132, 32, 17, 23, 3, 1)]


@pytest.mark.parametrize("teams", [0, 2])
@pytest.mark.parametrize("shape", WG3_SHAPES, ids=sid)
def test_impulse_wgrad_bf16_kernel_with_fp32_redo(shape, teams):
    """accumulate bits 1-2 clear, Cin, Cout, ldx, ldg multiples of 4: evf_conv2d_wgrad takes evf_wgrad9_b3_launch (k_wgrad9_b3, or the
    two-team k_wgrad9_b3v under evf_wgrad_teams_select(2) where CT = NT = 2: 72 -> 100 and 64 -> 128 channels), then k_wgrad9 with
    the redo flags, then the slab reduction.  The kernels flag per redo tile of 32 * CT input channels (64 once Cin > 32): Cin 32, 36
    and 64 are ONE tile holding exactly one full value; 72 -> 100 has an all-exact tile (channels 0..63) beside the flagged one
    (64..71) and 132 -> 32 a flagged tile between two exact ones -- the case the flags exist for.  A missed flag leaves the full value
    rounded to bf16, 2^-9 of its products."""
    wgrad_impulse_route(f"wgrad bf16 + redo teams {teams}", shape, 0, R.K_IMP, False, teams=teams)


@pytest.mark.parametrize("shape", WG3_SHAPES, ids=sid)
def test_impulse_wgrad_fp32_only(shape):
    """accumulate bit 1 (value 2): k_wgrad9 alone (csrc/evf_wgrad_gen.hip), K = 1 (accumulating: one unit per rounding of fl(x g) + old);
    pixel strides C + 3: its scalar loaders."""
    wgrad_impulse_route("wgrad fp32", shape, 2, R.K_F32, True, ld_pad=3)


@pytest.mark.parametrize("shape", WG3_SHAPES, ids=sid)
def test_impulse_wgrad_promise(shape):
    """accumulate bit 2 (value 4) on all-exact impulses: the bf16 kernel without the fp32 verification pass."""
    wgrad_impulse_route("wgrad promise", shape, 4, R.K_IMP, False, kinds="exact")


def test_impulse_wgrad_four_channel_head():
    """(2,4,32,24,40,3,1) inside ldx = 12, no bias gradient: wg_fewin_ok -> k_wgrad9_fewin (fp32 FMAs, K = 1)."""
    shape = (2, 4, 32, 24, 40, 3, 1)
    Bn, Cin, Cout, H, W, k, s = shape
    B = Bufs()
    rng = np.random.default_rng(12)
    case = R.wgrad_case(shape, wgrad_nsplit(shape))
    ref, hit, mag = case["ref"], case["hit"], np.abs(case["ref"])
    xw = rng.standard_normal((Bn, H, W, 12)).astype(F32)  # the activation is wider: channels 4.. belong to another product
    xw[..., :4] = case["x"]
    got, _ = wgrad_call(B, case, shape, flags=2, gw_init=np.full(ref.shape, FILL, F32), ldx=12, x_full=xw)
    check_wgrad("impulse", "wgrad four-channel head", "overwrite in ldx 12", got, ref, mag, R.K_F32, hit)
    base = rng.standard_normal((Cout, 12, 3, 3)).astype(F32)
    got, _ = wgrad_call(B, case, shape, flags=1 | 2, gw_init=base, cin_total=12, ldx=12, x_full=xw)
    check_wgrad("impulse", "wgrad four-channel head", "accumulate in a 12-channel weight", got, ref, mag, R.K_F32, hit, base=base, Cin=4, chain=True)
    B.check()


@pytest.mark.parametrize("shape,ws", [((1, 32, 2, 17, 33, 1, 1), "plan"), ((1, 32, 2, 17, 33, 1, 1), None), ((1, 32, 5, 17, 33, 1, 1), "plan"),
                                      ((3, 128, 4, 7, 5, 1, 1), "plan"), ((2, 6, 8, 12, 10, 5, 1), "plan"), ((1, 16, 16, 14, 14, 7, 2), "plan")],
                         ids=["1x1-streaming", "1x1-atomic", "1x1-matrix-core", "1x1-128-to-4", "5x5", "7x7-stride-2"])
def test_impulse_wgrad_1x1_and_larger_kernels(shape, ws):
    """1x1 with Cout <= 4 and scratch: wg1_small_ok -> k_wgrad1_small + k_wgrad1_reduce; with null scratch, with 5 outputs, and 5x5 /
    7x7: the general fp32 weight-gradient kernel (atomic split-K).  All fp32: K = 1 (accumulating: one unit per rounding)."""
    name = {1: "1x1", 5: "5x5", 7: "7x7"}[shape[5]]
    wgrad_impulse_route(f"wgrad {name} Cout {shape[2]}" + ("" if ws else " null scratch"), shape, 0, R.K_F32, True, ld_pad=4 if shape[5] == 1 else 3, ws=ws)


# ================================================================================================================ dense leg
DENSE_ROUTES = [
    ("general b3", (2, 66, 16, 10, 13, 3, 1), True, 0, 0, False, 0),
    ("general b3 stride 2", (3, 5, 7, 11, 13, 3, 2), True, 0, 0, False, 0),
    ("general b3 split", (1, 16, 16, 15, 15, 7, 2), True, 0, 3, False, 0),
    ("fp32", (2, 66, 16, 10, 13, 3, 1), False, -1, 0, False, 0),
    ("tile", (1, 20, 96, 18, 34, 3, 1), True, 2, 0, False, 0),
    ("tile split", (1, 20, 96, 18, 34, 3, 1), True, 2, 3, False, 0),
    ("n-stream", (2, 32, 132, 9, 33, 3, 1), True, 2, 0, True, 0),
    ("n-stream split", (1, 64, 260, 9, 33, 3, 1), True, 2, 3, True, 0),
    ("whole-image", (1, 96, 64, 13, 16, 3, 1), True, 2, 0, False, 0),
    ("whole-image split", (1, 96, 64, 13, 16, 3, 1), True, 2, 3, False, 0),
    ("promise", (2, 132, 32, 80, 130, 3, 1), True, -1, 0, False, 4 | (4 << 4)),
]


@pytest.mark.parametrize("route,shape,b3,tile,split,nstream,flags", DENSE_ROUTES, ids=[r[0].replace(" ", "-") for r in DENSE_ROUTES])
def test_dense_forward_and_input_gradient(route, shape, b3, tile, split, nstream, flags, monkeypatch):
    """Random operands through each route (real-valued, spike-valued, spikes behind a real-valued head), accumulating into a base with
    a bias on the forward: every element within K_SUM * 2^-24 * (sum |x||w| + |bias| + |base|) of float64."""
    Bn, Cin, Cout, H, W, k, s = shape
    for direction in ("fwd",) if flags else ("fwd", "dgrad"):
        select(monkeypatch, tile, split, nstream)
        B = Bufs()
        rng = np.random.default_rng(Cin + Cout)
        c = Conv(B, shape, direction, b3, rng, flags)
        base = rng.standard_normal(c.out_shape).astype(F32)
        bias = rng.standard_normal(c.N).astype(F32) if c.fwd else None
        for kind in ("mixed", "spikes") if flags else ("real", "spikes", "mixed"):
            src = R.dense_inputs(rng, c.src_shape, kind)
            if c.fwd:
                ref, scale = R.conv_fwd64(src, c.w, s) + bias, R.conv_fwd64(np.abs(src), np.abs(c.w), s) + np.abs(bias)
            else:
                ref, scale = R.conv_dgrad64(src, c.w, s, H, W), R.conv_dgrad64(np.abs(src), np.abs(c.w), s, H, W)
            got = c.run(src, base, bias=bias, acc=1, ld_pad=4)
            within("dense", f"{route} {direction}", kind, got, ref + base, scale + np.abs(base), R.K_SUM)
        B.check()


# route (named as in the impulse leg), shape, accumulate flags, teams, scratch ("plan" / None), four-channel head inside ldx = 12
DENSE_WGRAD = [("wgrad bf16 + redo teams 0", (2, 72, 100, 17, 23, 3, 1), 0, 0, "plan", False),
               ("wgrad bf16 + redo teams 2", (2, 72, 100, 17, 23, 3, 1), 0, 2, "plan", False),
               ("wgrad fp32", (2, 72, 100, 17, 23, 3, 1), 2, 0, "plan", False),
               ("wgrad promise", (2, 72, 100, 17, 23, 3, 1), 4, 0, "plan", False),
               ("wgrad stride 2", (2, 32, 64, 12, 12, 3, 2), 0, 0, "plan", False),
               ("wgrad four-channel head", (2, 4, 32, 24, 40, 3, 1), 2, 0, "plan", True),
               ("wgrad 1x1 Cout 2", (1, 32, 2, 17, 33, 1, 1), 0, 0, "plan", False),
               ("wgrad 1x1 Cout 2 null scratch", (1, 32, 2, 17, 33, 1, 1), 0, 0, None, False),
               ("wgrad 1x1 Cout 4", (3, 128, 4, 7, 5, 1, 1), 0, 0, "plan", False),
               ("wgrad 1x1 Cout 5", (1, 32, 5, 17, 33, 1, 1), 0, 0, "plan", False),
               ("wgrad 5x5 Cout 8", (2, 6, 8, 12, 10, 5, 1), 0, 0, "plan", False),
               ("wgrad 7x7 Cout 16", (1, 16, 16, 14, 14, 7, 2), 0, 0, "plan", False)]


@pytest.mark.parametrize("route,shape,flags,teams,ws,head", DENSE_WGRAD, ids=[r[0].replace(" ", "-") for r in DENSE_WGRAD])
def test_dense_weight_gradient(route, shape, flags, teams, ws, head):
    """Dense g_y against real-valued x, spike-valued x, and spike-valued x with ONE real value (one flagged redo tile beside an exact
    one: the per-tile redo flags): every element of g_w and g_bias within K_SUM * 2^-24 * sum |x||g| of float64 -- the sum over all
    pixels of every route, which the impulse leg (one product per element) does not hold.  The four-channel head (k_wgrad9_fewin:
    every image, row segment and interior pixel) runs inside a 12-channel activation and has no bias gradient."""
    Bn, Cin, Cout, H, W, k, s = shape
    assert _lib.load().evf_wgrad_teams_select(teams) == 0
    B = Bufs()
    rng = np.random.default_rng(Cin + 3 * Cout)
    OH, OW = R.out_dim(H, k, s), R.out_dim(W, k, s)
    gy = (rng.standard_normal((Bn, OH, OW, Cout)) * 0.5).astype(F32)
    everything = np.ones((Cout, Cin, k, k), bool)
    for kind in ("spikes",) if flags & 4 else ("real", "spikes", "one real value"):  # (a promise holds for spike-valued x only)
        x = R.dense_inputs(rng, (Bn, H, W, Cin), "real" if kind == "real" else "spikes")
        if kind == "one real value":
            x[Bn - 1, H // 2, W // 3, min(Cin - 1, 37)] = F32(0.3)
        case = {"x": x, "gy": gy}
        kw = {}
        if head:  # the activation is wider: channels 4.. belong to another product
            xw = rng.standard_normal((Bn, H, W, 12)).astype(F32)
            xw[..., :Cin] = x
            kw = {"ldx": 12, "x_full": xw}
        got, gb = wgrad_call(B, case, shape, flags=flags, gw_init=np.full((Cout, Cin, k, k), FILL, F32),
                             gb_init=None if head else np.full(Cout, FILL, F32), ws=ws, **kw)
        check_wgrad("dense", route, kind, got, R.conv_wgrad64(x, gy, k, s), R.conv_wgrad64(np.abs(x), np.abs(gy), k, s), R.K_SUM, everything)
        if not head:
            within("dense", route + " bias gradient", kind, gb, gy.astype(F64).sum((0, 1, 2)), np.abs(gy.astype(F64)).sum((0, 1, 2)), R.K_SUM)
    B.check()
