"""Host side of the streaming inference (event_flow_amd/stream.py) without a GPU: the push planner against a brute-force
simulation of the ring, the refusals that need no device, and the guards of evf_ring_append / evf_ring_cut as a sanitized
stand-alone program."""

import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_host_eval_steps import _Fused, _General

from event_flow_amd import _lib
from event_flow_amd.stream import FlowStream, check_events, plan_push, stream_refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def simulate(pushes, N, R, slots):
    """The planner's operations applied to a ring of event NUMBERS, one stream of consecutive pushes -> the windows run.  Checks
    on the way: a slice fits the ring, never overwrites an event of a window that is not cut yet, every window finds exactly its
    events, the windows of one push land in different result rows."""
    ring = np.full(R, -1, dtype=np.int64)
    appended = windows = 0
    ran = []
    for n in pushes:
        pending = appended - windows * N
        ops = plan_push(pending, n, N, R, slots, windows)
        at, rows = 0, []
        for op in ops:
            if op[0] == "append":
                _, lo, hi = op
                assert lo == at and lo < hi <= n and hi - lo <= R
                ids = np.arange(appended, appended + hi - lo)
                old = ring[ids % R]
                assert np.all(old < windows * N), "a slice overwrites an event of an uncut window"
                ring[ids % R] = ids
                appended += hi - lo
                at = hi
            else:
                _, k, first, row = op
                assert (k, first, row) == (windows, windows * N, windows % slots)
                assert first + N <= appended and first >= appended - R  # evf_ring_cut's own guard
                assert np.array_equal(ring[np.arange(first, first + N) % R], np.arange(first, first + N))
                windows += 1
                rows.append(row)
                ran.append(k)
        assert at == n and len(set(rows)) == len(rows)
        assert 0 <= appended - windows * N < N  # every complete window ran
    return ran, appended


def test_planner_against_a_brute_force_ring():
    rng = np.random.Generator(np.random.PCG64(21))
    cases = 0
    for _ in range(300):
        N = int(rng.integers(1, 40))
        R = int(N + rng.integers(0, 3 * N + 2))
        slots = int(rng.integers(1, 6))
        pushes, pending = [], 0
        for _k in range(int(rng.integers(1, 12))):
            most = slots * N - pending
            kind = rng.integers(0, 5)
            if kind == 0:
                n = most  # the largest push accepted
            elif kind == 1:
                n = min(most, N - pending)  # ends exactly on a window border
            elif kind == 2:
                n = min(most, (R - (sum(pushes) % R)) % R)  # ends exactly on the ring's end
            else:
                n = int(rng.integers(0, most + 1))
            pushes.append(n)
            pending = (pending + n) % N
        ran, appended = simulate(pushes, N, R, slots)
        assert appended == sum(pushes) and ran == list(range(sum(pushes) // N))
        cases += 1
    assert cases == 300


def test_planner_examples_and_refusals():
    assert plan_push(0, 0, 10, 25, 8) == []
    assert plan_push(0, 10, 10, 10, 1) == [("append", 0, 10), ("window", 0, 0, 0)]  # a ring of one window
    assert plan_push(3, 30, 10, 25, 8, 2) == [("append", 0, 22), ("window", 2, 20, 2), ("window", 3, 30, 3), ("append", 22, 30),
                                              ("window", 4, 40, 4)]
    assert plan_push(9, 1, 10, 12, 2, 7) == [("append", 0, 1), ("window", 7, 70, 1)]
    assert len([op for op in plan_push(5, 8 * 10 - 5, 10, 25, 8) if op[0] == "window"]) == 8  # the largest push accepted
    with pytest.raises(_lib.EvflowError, match="push at most 75 events"):
        plan_push(5, 76, 10, 25, 8)
    for bad in ((10, 1, 10, 25, 8), (-1, 1, 10, 25, 8)):
        with pytest.raises(_lib.EvflowError, match="pending"):
            plan_push(*bad)
    for bad in ((0, 1, 10, 9, 8), (0, 1, 0, 9, 8), (0, 1, 10, 25, 0)):
        with pytest.raises(_lib.EvflowError, match="ring of"):
            plan_push(*bad)


def test_event_checks_need_no_device():
    H, W = 6, 9
    x, y, t, p = np.array([0, 8, 3]), np.array([5, 0, 2]), np.array([0.5, 0.75, 1.0]), np.array([0, 1, 1])
    cx, cy, ct, cp = check_events(x, y, t, p, H, W)
    assert (cx.dtype, cy.dtype, ct.dtype, cp.dtype) == (np.uint16, np.uint16, np.float64, np.uint8)
    assert cx.tolist() == [0, 8, 3] and cp.tolist() == [0, 1, 1]
    check_events(x.astype(np.float32), y.astype(np.float64), t, p.astype(bool), H, W)  # integers in float columns, as the files hold
    with pytest.raises(_lib.EvflowError, match=r"xs .* \[0, 9\)"):
        check_events(np.array([0, W, 3]), y, t, p, H, W)
    with pytest.raises(_lib.EvflowError, match=r"ys .* \[0, 6\)"):
        check_events(x, np.array([0, -1, 3]), t, p, H, W)
    with pytest.raises(_lib.EvflowError, match="no integers"):
        check_events(np.array([0, 1.5, 3]), y, t, p, H, W)
    with pytest.raises(_lib.EvflowError, match="polarities"):
        check_events(x, y, t, np.array([0, 2, 1]), H, W)
    for bad in (np.nan, np.inf):
        with pytest.raises(_lib.EvflowError, match="not finite"):
            check_events(x, y, np.array([0.5, bad, 1.0]), p, H, W)
    with pytest.raises(_lib.EvflowError, match="equal length"):
        check_events(x, y[:2], t, p, H, W)
    with pytest.raises(_lib.EvflowError, match="equal length"):
        check_events(x.reshape(3, 1), y, t, p, H, W)


def test_stream_refusals_name_the_eager_alternative(monkeypatch):
    assert stream_refusal(_FusedNet()) is None
    why = stream_refusal(_General())
    assert "general path" in why and "ConvGRU" in why and "encode_event_list" in why
    why = stream_refusal(object())
    assert "no fused FireNet engine" in why and "encode_event_list" in why
    assert "has no state_buffers" in stream_refusal(_Fused())
    monkeypatch.setenv("WORLD_SIZE", "4")
    why = stream_refusal(_FusedNet())
    assert "WORLD_SIZE = 4" in why and "encode_event_list" in why
    assert stream_refusal(_FusedNet(), world_size=1) is None


class _FusedNet(_Fused):
    state_buffers = set_state_buffers = final_states_into = mark_last_pass = None


def test_flow_stream_refuses_before_any_device_work(monkeypatch):
    """A general-path network and WORLD_SIZE > 1: raised by the constructor before anything touches the device."""
    from event_flow_amd.models.model import FireNet, LIFFireNet
    from test_host_activity import _model_cfg

    def no_device(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    config = {"loader": {"resolution": [8, 8]}, "hot_filter": {"enabled": False}}
    ann = FireNet({**_model_cfg(), "activations": ["relu", None], "spiking_neuron": None})
    lif = LIFFireNet(_model_cfg())
    for name in ("Stream", "Event", "is_available", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    monkeypatch.setattr(torch, "zeros", no_device)
    with pytest.raises(_lib.EvflowError, match="general path.*encode_event_list"):
        FlowStream(ann, config, window=100)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(_lib.EvflowError, match="WORLD_SIZE = 2.*encode_event_list"):
        FlowStream(lif, config, window=100)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(_lib.EvflowError, match="at least one window"):
        FlowStream(lif, config, window=100, capacity=99)


def test_launcher_guards_as_a_sanitized_stand_alone_program(tmp_path):
    """tools/stream_guards.cpp with csrc/evf_stream.hip, host code under AddressSanitizer and UBSan: every EVF_EINVAL case is
    answered before any launch (the program makes no accepted call that launches)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc to build tools/stream_guards.cpp with")
    exe = str(tmp_path / "stream_guards")
    cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "event_flow_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "stream_guards.cpp"), os.path.join(ROOT, "event_flow_amd", "csrc", "evf_stream.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
    assert "all guards answered EVF_EINVAL before any launch" in ran.stdout
