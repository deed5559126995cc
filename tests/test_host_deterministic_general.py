"""Deterministic mode on the spiking general path, what can be checked without a GPU: the scratch sizes of
evf_neuron_bwd_det / evf_clip_adam_step_det against the launch geometry of tests/neuron_gen_ref.py, their refusals, the size
hip_ops allocates, and the ctypes table."""

import neuron_gen_ref as R
from event_flow_amd import _lib, build


def lib():
    build.build(verbose=False)
    return _lib.load()


def test_neuron_scratch_holds_one_row_per_block():
    L = lib()
    for C, npix in R.SMALL_SHAPES + R.BLOCK_SHAPES:
        g = R.bwd_geometry(C, npix)
        for kind, name in enumerate(R.KINDS):
            n_par = 2 if name == "lif" else 4
            assert L.evf_neuron_bwd_det_ws(npix, C, kind) >= g["nblk"] * n_par * C, (C, npix, name)


def test_neuron_scratch_is_zero_for_what_the_call_refuses():
    L = lib()
    assert L.evf_neuron_bwd_det_ws(70, 32, 0) > 0
    for npix, C, kind in ((70, 6, 0), (70, 30, 1), (70, 1028, 0), (70, 0, 0), (0, 32, 0), (-5, 32, 2), (70, 32, 4), (70, 32, -1)):
        assert L.evf_neuron_bwd_det_ws(npix, C, kind) == 0, (npix, C, kind)


def test_hip_ops_allocates_the_largest_neuron_scratch():
    from event_flow_amd.models import hip_ops

    L = lib()
    sizes = [L.evf_neuron_bwd_det_ws(npix, C, kind) for kind in range(4) for C in range(4, 1025, 4)
             for npix in (1, 63, 4097, 1 << 16, 1 << 20, 1 << 26)]
    assert max(sizes) == hip_ops.NEURON_DET_WS_FLOATS == 1024 * 4 * 1024


def test_adam_partials_hold_one_sum_per_block():
    L = lib()
    for n in (1, 256, 1 << 20, 25_000_000):
        blocks = min(-(-n // 256), 1024)  # the grid of the two-launch step (evf_clip_adam_step)
        assert blocks <= L.evf_clip_adam_det_ws(n) <= 1024, n
    assert L.evf_clip_adam_det_ws(0) == 0 and L.evf_clip_adam_det_ws(-3) == 0


def test_fused_fits_needs_no_gpu():
    L = lib()
    assert L.evf_clip_adam_fused_fits(1 << 20, 4096) == 1 and L.evf_clip_adam_fused_fits((1 << 20) + 1, 4096) == 0
    assert L.evf_clip_adam_fused_fits(1024, 4100) == 0 and L.evf_clip_adam_fused_fits(0, 4096) == 0


def test_signatures_of_the_new_entry_points():
    P, I, F, Lg = _lib.P, _lib.I, _lib.F, _lib.L
    S = _lib.SIGNATURES
    # evf_neuron_bwd's arguments, ws followed by its size in floats (the stream last)
    bwd = S["evf_neuron_bwd"]
    assert S["evf_neuron_bwd_det"] == bwd[:-1] + [Lg, P]
    assert S["evf_neuron_bwd_det_ws"] == [Lg, I, I]
    step = S["evf_clip_adam_step"]
    assert S["evf_clip_adam_step_det"] == step[:-1] + [P, Lg, P]
    assert S["evf_clip_adam_det_ws"] == [Lg]
    assert S["evf_clip_adam_fused_fits"] == [Lg, P]
    for name in ("evf_neuron_bwd_det_ws", "evf_clip_adam_det_ws"):
        assert _lib.RESTYPES[name] is _lib.ctypes.c_int64
