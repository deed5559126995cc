"""Deterministic mode for the non-spiking zoo, what can be checked without a GPU: the scratch sizes of evf_chan_reduce_det /
evf_leaky_bwd_det / evf_conv2d_wgrad_det against the geometry twins of tests/zoo_det_ref.py, their zero for what the calls
refuse, the ctypes table, the scratch hip_ops allocates, and the float32 emulations of the kernels' association against the
float64 references at the bounds of the GPU tests, on the GPU tests' own inputs: the references alone stay inside the bar."""

import numpy as np
import pytest
import torch

import conv_ref as CR
import neuron_gen_ref as R
import zoo_det_ref as Z
from event_flow_amd import _lib, build

F32, F64 = np.float32, np.float64


def lib():
    build.build(verbose=False)
    return _lib.load()


def inside(got, ref, scale, k, extra=0.0):
    err = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    bound = k * Z.U * (np.asarray(scale, F64) + extra)
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
    return float(np.max(err / np.maximum(bound, 1e-300)))


# ================================================================================================================ scratch sizes
def test_scratch_holds_rows_times_columns_of_the_twin_geometry():
    L = lib()
    for G in Z.CHAN_G + (8,):
        for npg in Z.CHAN_NPG + (1, 64 * 64, 1 << 20):
            for C in Z.CHAN_C + (1, 64, 512):
                g = Z.chan_geometry(G, npg, C)
                assert g["bpg"] * g["ppb"] >= npg
                assert L.evf_chan_reduce_det_ws(G, npg, C) >= G * g["rows"] * g["cols"], (G, npg, C)
    for Cout in Z.BIAS_COUT:
        g = Z.chan_geometry(1, Z.BIAS_M, Cout)
        assert L.evf_chan_reduce_det_ws(1, Z.BIAS_M, Cout) >= g["rows"] * Cout
    for C, npix in R.SMALL_SHAPES + R.BLOCK_SHAPES:
        g = Z.leaky_geometry(C, npix)
        assert g["nblk"] * g["bs"] * g["trips"] >= npix * g["Q"]
        assert L.evf_leaky_bwd_det_ws(npix, C) >= g["rows"] * g["cols"], (C, npix)
    for shape in Z.WGRAD_SHAPES + (Z.WGRAD_OFFSET_CASE[0],):
        g = Z.wgrad_det_geometry(*shape)
        assert g["ksplit"] * g["stages"] * 32 >= g["M"]
        assert L.evf_conv2d_wgrad_det_ws(*shape) >= g["rows"] * g["cols"], shape
    assert any(Z.wgrad_det_geometry(*s)["ksplit"] > 1 for s in Z.WGRAD_SHAPES)
    assert {(Z.wgrad_det_geometry(*s)["CT"], Z.wgrad_det_geometry(*s)["NT"]) for s in Z.WGRAD_SHAPES} == {(1, 1), (2, 2), (2, 1)}
    # what forwards to the default entry needs the default's scratch
    assert L.evf_conv2d_wgrad_det_ws(*Z.WGRAD_FORWARD_CASE) == L.evf_conv2d_wgrad_ws(*Z.WGRAD_FORWARD_CASE) > 0
    assert L.evf_conv2d_wgrad_det_ws(2, 20, 24, 32, 2, 1, 1) >= L.evf_conv2d_wgrad_ws(2, 20, 24, 32, 2, 1, 1) > 0
    assert L.evf_conv2d_wgrad_det_ws(2, 20, 24, 4, 32, 3, 1) == L.evf_conv2d_wgrad_ws(2, 20, 24, 4, 32, 3, 1) > 0


def test_scratch_is_zero_for_what_the_calls_refuse():
    L = lib()
    assert L.evf_chan_reduce_det_ws(1, 700, 32) > 0
    for G, npg, C in ((0, 700, 32), (-1, 700, 32), (1, 0, 32), (1, -4, 32), (1, 700, 0), (1, 700, -3)):
        assert L.evf_chan_reduce_det_ws(G, npg, C) == 0, (G, npg, C)
    assert L.evf_leaky_bwd_det_ws(70, 32) > 0
    for npix, C in ((70, 6), (70, 30), (70, 1028), (70, 0), (0, 32), (-5, 32)):
        assert L.evf_leaky_bwd_det_ws(npix, C) == 0, (npix, C)
    assert L.evf_conv2d_wgrad_det_ws(2, 20, 24, 9, 11, 5, 1) > 0
    for shape in ((0, 20, 24, 9, 11, 5, 1), (2, 0, 24, 9, 11, 5, 1), (2, 20, 0, 9, 11, 5, 1), (2, 20, 24, 0, 11, 5, 1),
                  (2, 20, 24, 9, 0, 5, 1), (2, 20, 24, 9, 11, 4, 1), (2, 20, 24, 9, 11, 9, 1), (2, 20, 24, 9, 11, 5, 3),
                  (2, 20, 24, 9, 11, 5, 0)):
        assert L.evf_conv2d_wgrad_det_ws(*shape) == 0, shape


def test_ctypes_table_has_the_six_entry_points():
    S, P, I, Lg = _lib.SIGNATURES, _lib.P, _lib.I, _lib.L
    red = S["evf_chan_reduce"]  # its arguments, then accumulate, ws and its size in floats (the stream last)
    assert S["evf_chan_reduce_det"] == red[:-1] + [I, P, Lg, P]
    assert S["evf_chan_reduce_det_ws"] == [I, Lg, I]
    assert S["evf_leaky_bwd_det"] == S["evf_leaky_bwd"][:-1] + [P, Lg, P]
    assert S["evf_leaky_bwd_det_ws"] == [Lg, I]
    wg = S["evf_conv2d_wgrad"]  # (ends with ws, stream): the size follows ws
    assert S["evf_conv2d_wgrad_det"] == wg[:-1] + [Lg, P]
    assert S["evf_conv2d_wgrad_det_ws"] == S["evf_conv2d_wgrad_ws"]
    for name in ("evf_chan_reduce_det_ws", "evf_leaky_bwd_det_ws", "evf_conv2d_wgrad_det_ws"):
        assert _lib.RESTYPES[name] is _lib.ctypes.c_int64
    L = lib()
    for name in ("evf_chan_reduce_det", "evf_leaky_bwd_det", "evf_conv2d_wgrad_det"):
        assert getattr(L, name).restype is _lib.ctypes.c_int


def test_hip_ops_scratch_sizing():
    from event_flow_amd.models import hip_ops

    assert hip_ops.det_ws_floats(0) == hip_ops.det_ws_floats(1) == hip_ops.DET_WS_MIN_FLOATS
    for n in (hip_ops.DET_WS_MIN_FLOATS, hip_ops.DET_WS_MIN_FLOATS + 1, 195264, 1 << 20, (1 << 20) + 1, 1024 * 1024 * 4):
        size = hip_ops.det_ws_floats(n)
        assert n <= size < 2 * max(n, hip_ops.DET_WS_MIN_FLOATS) and size & (size - 1) == 0, n
    dev = torch.device("cpu")  # (the bookkeeping does not care where the buffer lives)
    try:
        a = hip_ops._det_ws("test", 10, dev)
        assert a.numel() == hip_ops.DET_WS_MIN_FLOATS and a.dtype == torch.float32
        assert hip_ops._det_ws("test", 5000, dev) is a  # one buffer per device and kind, reused
        assert hip_ops._det_ws("other", 10, dev) is not a
        b = hip_ops._det_ws("test", a.numel() + 1, dev)  # grown on demand
        assert b is not a and b.numel() == 2 * a.numel()
        assert any(r is a for r in hip_ops._DET_WS_RETIRED)  # (captured graphs may still hold the outgrown buffer's address)
        assert hip_ops._det_ws("test", 10, dev) is b
    finally:
        hip_ops._DET_WS.pop((dev, "test"), None)
        hip_ops._DET_WS.pop((dev, "other"), None)
        hip_ops._DET_WS_RETIRED[:] = [r for r in hip_ops._DET_WS_RETIRED if r.device.type != "cpu"]


# ============================================================================================ the emulations inside the bounds
@pytest.mark.parametrize("npg", Z.CHAN_NPG)
@pytest.mark.parametrize("C", Z.CHAN_C)
def test_chan_reduce_emulation_inside_the_bound(C, npg):
    for G in Z.CHAN_G:
        chain = Z.chan_geometry(G, npg, C)["chain"]
        for pad in (0, 4):
            x, y, center, scale, init = Z.chan_inputs(G, npg, C, pad)
            for mode in (0, 1, 2):
                ref, sab = Z.chan_ref64(x, y, center, scale, mode, G, npg, C)
                k = Z.CHAN_OPS[mode] + chain
                inside(Z.chan_emulate32(x, y, center, scale, mode, G, npg, C), ref, sab, k)
                inside(Z.chan_emulate32(x, y, center, scale, mode, G, npg, C, init), ref + init, sab, k, extra=np.abs(init.astype(F64)))


@pytest.mark.parametrize("Cout", Z.BIAS_COUT)
def test_bias_emulation_inside_the_project_bar(Cout):
    gy, init = Z.bias_inputs(Cout)
    ref, sab = Z.chan_ref64(gy, None, None, None, 0, 1, Z.BIAS_M, Cout)
    assert inside(Z.chan_emulate32(gy, None, None, None, 0, 1, Z.BIAS_M, Cout), ref, sab, CR.K_SUM) < 1.0
    inside(Z.chan_emulate32(gy, None, None, None, 0, 1, Z.BIAS_M, Cout, init[None]), ref + init, sab, CR.K_SUM, extra=np.abs(init.astype(F64)))


@pytest.mark.parametrize("C,npix", R.SMALL_SHAPES + R.BLOCK_SHAPES)
def test_leaky_emulation_inside_the_bound(C, npix):
    d = Z.leaky_inputs(C, npix)
    chain = Z.leaky_geometry(C, npix)["chain"]
    big = npix > 1000
    for _, act in Z.LEAKY_ACTS[:1] if big else Z.LEAKY_ACTS:
        for has_prev in (True,) if big else (True, False):
            prev = d["prev"] if has_prev else None
            mix = Z.leaky_mix32(d["cur"], prev, d["leak"])
            for up in Z.LEAKY_UPSTREAM[:1] if big else Z.LEAKY_UPSTREAM:
                go = d["g_out"] if up in ("both", "out") else None
                gs = d["g_state"] if up in ("both", "state") else None
                ref = Z.leaky_reference(mix, prev, d["leak"], act, go, gs)
                got = Z.leaky_emulate32(mix, prev, d["leak"], act, go, gs, d["init"])
                inside(got, d["init"].astype(F64) + ref["g_leak"], ref["s_g_leak"], R.K_LEAKY + chain, extra=np.abs(d["init"].astype(F64)))


@pytest.mark.parametrize("shape", Z.WGRAD_SHAPES)
def test_wgrad_emulation_inside_the_project_bar(shape):
    k, s = shape[5], shape[6]
    x, gy = Z.wgrad_inputs(shape)
    inside(Z.wgrad_emulate32(x, gy, k, s), CR.conv_wgrad64(x, gy, k, s), CR.conv_wgrad64(np.abs(x), np.abs(gy), k, s), CR.K_SUM)
