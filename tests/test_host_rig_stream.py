"""Host side of the rig stream (event_flow_amd/rig_stream.py) without a GPU: `plan_tick` and `RigPlan` against a brute-force
restatement of the borders, against `ResidentEvalPlan` in `time` mode on sequence files, the refusals with the counters unchanged,
the table layout, and the guards of evf_rings_append / evf_rings_cut_ragged as a sanitized stand-alone program."""

import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_host_loader import _cfg

from event_flow_amd import _lib
from event_flow_amd.dataloader.h5 import write_npz_sequence
from event_flow_amd.dataloader.resident_eval import ResidentEvalPlan
from event_flow_amd.rig_stream import RigPlan, RigStream, _TickTable, border_index, plan_tick, table_words, window_borders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (16, 20)
BIG = 10 ** 6


def brute(lists, t0, dt, watermark=-np.inf):
    """The windows of per-camera ascending timestamp lists, restated: the cursor `row += dt`, window k = the events with
    row + t0 <= ts < (row + t0) + dt, first = the number of events before the opening border, up to 10 events are none; a window
    runs when every camera's last timestamp (or the watermark) has reached its closing border -> per window [(first, count)]."""
    row, out = 0.0, []
    while True:
        begin = row + t0
        end = begin + dt
        if any(max(ts[-1] if len(ts) else -np.inf, watermark) < end for ts in lists):
            return out
        jobs = []
        for ts in lists:
            n = sum(1 for t in ts if begin <= t < end)
            jobs.append((sum(1 for t in ts if t < begin), n if n > 10 else 0))
        out.append(jobs)
        row += dt


def run_plan(plan, lists, chunks, rng=None, watermark=None):
    """Push `lists` through `plan` in pushes of chunks() events per camera (then the watermark) -> per window [(first, count)]."""
    out, at = [], [0] * len(lists)
    while any(a < len(ts) for a, ts in zip(at, lists)):
        take = [min(int(chunks()), len(ts) - a) for a, ts in zip(at, lists)]
        state, heads, ticks = plan.plan(ts=[np.asarray(ts[a:a + n], dtype=np.float64) for ts, a, n in zip(lists, at, take)])
        assert heads == at
        plan.commit(state)
        at = [a + n for a, n in zip(at, take)]
        out += ticks
    if watermark is not None:
        state, _heads, ticks = plan.plan(advance=watermark)
        plan.commit(state)
        out += ticks
    assert [t[0] for t in out] == list(range(len(out)))
    for k, row, jobs, appended, res_row in out:
        assert res_row == k % plan.slots
        for (first, count, dropped), a in zip(jobs, appended):
            assert dropped == 0 and 0 <= first and first + count <= a
    return [[j[:2] for j in t[2]] for t in out]


def test_plan_on_a_border_a_gap_and_windows_of_ten_and_eleven_events():
    t0, dt = 100.0, 0.25  # (borders that float64 holds exactly: 100.25, 100.5, ...)
    cam0 = ([100.0 + 0.02 * i for i in range(11)]               # window 0: 11 events
            + [100.25 + 0.02 * i for i in range(10)]            # window 1: 10 events -> cut as empty
            + [100.5] + [100.51 + 0.01 * i for i in range(19)]  # window 2: starts EXACTLY on its opening border, 20 events
            + [101.0 + 0.005 * i for i in range(30)]            # window 3: none (a gap) | window 4: 30 events
            + [101.25])                                         # exactly on window 4's closing border: it closes the window
    cam1 = [100.001 + 0.0101 * i for i in range(124)]           # a camera that runs on at its own rate (up to 101.2433)
    want = brute([cam0, cam1], t0, dt)
    assert [j[0] for j in want] == [(0, 11), (11, 0), (21, 20), (41, 0)]  # (window 4 waits for camera 1)
    plan = RigPlan(2, dt, 300, capacity=BIG, slots=BIG, t0=t0)
    assert run_plan(plan, [cam0, cam1], lambda: 7) == want
    state, _h, ticks = plan.plan(advance=101.25)  # the declaration completes window 4 for the idle camera
    plan.commit(state)
    assert [j[:2] for j in ticks[0][2]] == [(41, 30), (99, 25)] and len(ticks) == 1
    assert brute([cam0, cam1], t0, dt, watermark=101.25)[-1] == [(41, 30), (99, 25)]
    # the pure function itself: not complete -> None; the timestamp on the border belongs to the window it opens
    ts = [np.asarray(cam0), np.asarray(cam1)]
    assert plan_tick(ts, [0, 0], [100.2, 200.0], 0.0, t0, dt, 300) is None
    jobs, nxt = plan_tick(ts, [0, 0], [100.25, 100.25], 0.0, t0, dt, 300)
    assert nxt == 0.25 and jobs[0] == (0, 11, 0, 11) and jobs[1][:3] == (0, 25, 0)
    jobs, _ = plan_tick([t[11:] for t in ts], [11, 11], [200.0, 200.0], 0.5, t0, dt, 300)
    assert jobs[0][:3] == (21, 20, 0)
    assert border_index(np.array([1.0, 2.0, 2.0, 2.0, 3.0]), 2.0) == 1  # the leftmost of equal timestamps on a border
    assert window_borders(0.5, t0, dt) == (100.5, 100.75)
    # overflow: "raise" refuses, "newest" keeps the newest max_events and reports the rest
    with pytest.raises(_lib.EvflowError, match="max_events = 15.*overflow='newest'"):
        plan_tick(ts, [0, 0], [200.0, 200.0], 0.0, t0, dt, 15)
    jobs, _ = plan_tick(ts, [0, 0], [200.0, 200.0], 0.0, t0, dt, 15, overflow="newest")
    assert jobs[0][:3] == (0, 11, 0) and jobs[1][:3] == (10, 15, 10)


def test_plan_against_the_brute_force_restatement_on_random_lists():
    rng = np.random.Generator(np.random.PCG64(5))
    windows = 0
    for trial in range(40):
        B = int(rng.integers(1, 5))
        dt = float(rng.choice([0.1, 0.25, 0.037, 1.0 / 3.0]))  # (0.1: `row += dt` is not k * dt)
        t0 = float(rng.choice([0.0, 50.0, 1.5e9]))
        lists = []
        for _b in range(B):
            n = int(rng.integers(0, 400))
            ts = t0 + np.sort(rng.random(n)) * dt * float(rng.integers(1, 30))
            if n > 20:  # a gap of a few windows, duplicates, and one event exactly on a border of the cursor
                ts[n // 2:] += 3 * dt
                ts[5] = ts[4]
                row = 0.0
                for _k in range(int(rng.integers(1, 4))):
                    row += dt
                ts[n // 3] = row + t0
                ts = np.sort(ts)
            lists.append(ts.tolist())
        watermark = None if rng.integers(0, 2) and all(len(ts) for ts in lists) else t0 + dt * float(rng.integers(1, 40))
        want = brute(lists, t0, dt, -np.inf if watermark is None else watermark)
        plan = RigPlan(B, dt, 10 ** 4, capacity=BIG, slots=BIG, t0=t0)
        assert run_plan(plan, lists, lambda: rng.integers(0, 60), watermark=watermark) == want, trial
        windows += len(want)
    assert windows > 200


def _timed_files(path, B, t0, last, n=1500):
    """B sequence files with distinct timestamps that share t0 and duration -> (paths, timestamps)."""
    paths, cols = [], []
    for b in range(B):
        rng = np.random.Generator(np.random.PCG64(60 + b))
        inner = t0 + np.sort(rng.random(n - 2)) * (last - t0) * 0.999 + 1e-4
        if b == 1:  # the second camera is quiet for a while: empty windows in one camera only
            inner = inner[(inner < t0 + 0.62) | (inner > t0 + 0.95)]
        ts = np.concatenate([[t0], inner, [last]])
        m = len(ts)
        name = str(path / f"s{b}.npz")
        write_npz_sequence(name, rng.integers(0, RES[1], m), rng.integers(0, RES[0], m), ts, rng.integers(0, 2, m))
        paths.append(name)
        cols.append(ts)
    return paths, cols


@pytest.mark.parametrize("B", [1, 2])
def test_plan_equals_the_resident_eval_plan_in_time_mode(tmp_path, B):
    t0, last, dt = 100.0, 102.03, 0.1
    paths, cols = _timed_files(tmp_path, B, t0, last)
    ref = ResidentEvalPlan(_cfg(tmp_path, "time", dt, B, RES), 2)
    for p, ts in zip(paths, cols):  # what makes the reference's search and the leftmost rule provably the same
        assert np.all(np.diff(ts) > 0), "distinct timestamps"
        assert not np.any(ref.queries[p] == ts[-1]), "the last timestamp lies on no border"
        assert float(ref.meta[p]["t0"]) == t0 and ref.meta[p]["last_ts"] == last - t0
    want = []
    for i, (jobs, (restarted, done)) in enumerate(ref.plan_batches()):
        if done or (i > 0 and restarted):
            break
        assert [j[0] for j in jobs] == paths
        want.append([(j[1] if j[2] else None, j[2]) for j in jobs])
    assert len(want) == 20 and all(w[0][1] > 10 for w in want)
    assert B == 1 or any(w[1][1] == 0 for w in want)  # (an empty window in one camera only)
    rng = np.random.Generator(np.random.PCG64(9))
    for chunks in (lambda: 10 ** 5, lambda: 37, lambda: rng.integers(0, 300)):
        plan = RigPlan(B, dt, 10 ** 4, capacity=BIG, slots=BIG, t0=t0)
        got = run_plan(plan, [ts.tolist() for ts in cols], chunks)
        assert len(got) >= len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            for (gf, gc), (wf, wc) in zip(g, w):
                assert gc == wc and (wf is None or gf == wf), (k, g, w)  # (an empty window's first event is of no consequence)


def test_every_refusal_leaves_the_counters_unchanged():
    t0, dt = 10.0, 0.5
    plan = RigPlan(2, dt, 50, capacity=120, slots=3, t0=t0)
    a = 10.0 + 0.01 * np.arange(40)
    state, _h, ticks = plan.plan(ts=[a, a[:5]])
    assert not ticks
    plan.commit(state)
    before = plan.counters()
    assert plan.uncut == [40, 5] and plan.appended == [40, 5]
    more = 10.4 + 0.001 * np.arange(81)
    # camera 0 runs ahead while camera 1 lags: its ring would lose events of window 0
    with pytest.raises(_lib.EvflowError, match=r"camera 0 would overwrite.*waits for camera 1.*advance\(t\).*at most 80 events"):
        plan.plan(ts=[more, a[:0]])
    assert plan.counters() == before
    # more windows than result rows in one call
    with pytest.raises(_lib.EvflowError, match="more than 3 windows.*smaller steps.*more slots"):
        plan.plan(advance=t0 + 4 * dt)
    with pytest.raises(_lib.EvflowError, match="more than 3 windows"):
        plan.plan(ts=[np.array([10.5, 11.0, 11.5, 12.0]), np.array([12.0])])
    assert plan.counters() == before
    # timestamps that go backwards within a camera: against the last push, and inside a push
    with pytest.raises(_lib.EvflowError, match="camera 1's timestamps go backwards.*reset"):
        plan.plan(ts=[a[:0], np.array([10.03, 10.2])])
    with pytest.raises(_lib.EvflowError, match="camera 0's timestamps go backwards"):
        plan.plan(ts=[np.array([10.45, 10.44]), a[:0]])
    assert plan.counters() == before
    # a window fuller than max_events
    with pytest.raises(_lib.EvflowError, match="camera 0: .* holds 60 events, more than max_events = 50"):
        plan.plan(ts=[10.4 + 0.001 * np.arange(20), a[:0]], advance=t0 + dt)
    assert plan.counters() == before
    # one tuple per camera; a watermark that is no time
    with pytest.raises(_lib.EvflowError, match="per camera"):
        plan.plan(ts=[a])
    with pytest.raises(_lib.EvflowError, match="watermark"):
        plan.plan(advance=np.nan)
    assert plan.counters() == before
    # ... and the state still works: the largest push accepted, three windows in one call
    plan.plan(ts=[10.4 + 0.0001 * np.arange(80), a[:0]])
    assert plan.counters() == before  # (planned, not committed)
    state, _h, ticks = plan.plan(ts=[np.concatenate([10.4 + 0.001 * np.arange(9), [11.6]]), np.array([11.6])])
    assert [t[0] for t in ticks] == [0, 1, 2] and [t[4] for t in ticks] == [0, 1, 2]
    assert [j[:2] for j in ticks[0][2]] == [(0, 49), (0, 0)]
    # constructor refusals
    for bad in (dict(cameras=0), dict(cameras=17), dict(window_dt=0.0), dict(window_dt=np.inf), dict(max_events=0), dict(slots=0),
                dict(capacity=49), dict(overflow="oldest")):
        with pytest.raises(_lib.EvflowError, match="RigStream"):
            RigPlan(**{**dict(cameras=2, window_dt=dt, max_events=50), **bad})


def test_table_layout():
    for B in (1, 2, 3, 16):
        words = table_words(B)
        assert words == 2 * B + (3 * B + 2) // 2 + 1 and 8 * (words - 1) >= 16 * B + 4 * (3 * B + 1)
        jobs = [(1000 + b, 20 + b, 0) for b in range(B)]
        for reset in (False, True):
            tab = _TickTable("cpu", B)._job_table((jobs, [5000 + b for b in range(B)], reset, 6))
            assert tab.dtype == np.int64 and len(tab) == words
            assert tab[:B].tolist() == [1000 + b for b in range(B)] and tab[B:2 * B].tolist() == [5000 + b for b in range(B)]
            aux = tab[2 * B:].view(np.int32)
            assert aux[:B].tolist() == [20 + b for b in range(B)] and not aux[B:2 * B].any()  # counts | no flips
            assert aux[2 * B:3 * B + 1].tolist() == [int(reset)] * (B + 1)  # hot-pixel reset per camera | state reset
            assert tab[-1] == 6


def test_rig_stream_refuses_before_any_device_work(monkeypatch):
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
    with pytest.raises(_lib.EvflowError, match="RigStream.*general path.*encode_event_list"):
        RigStream(ann, config, cameras=2, window_dt=0.01, max_events=100)
    with pytest.raises(_lib.EvflowError, match="17 cameras"):
        RigStream(lif, config, cameras=17, window_dt=0.01, max_events=100)
    with pytest.raises(_lib.EvflowError, match="at least max_events"):
        RigStream(lif, config, cameras=2, window_dt=0.01, max_events=100, capacity=99)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(_lib.EvflowError, match="WORLD_SIZE = 2"):
        RigStream(lif, config, cameras=2, window_dt=0.01, max_events=100)


def test_launcher_guards_as_a_sanitized_stand_alone_program(tmp_path):
    """tools/rig_stream_guards.cpp with csrc/evf_stream.hip, host code under AddressSanitizer and UBSan: every EVF_EINVAL case of
    the two rig entry points is answered before any launch (the program makes no accepted call that launches)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc to build tools/rig_stream_guards.cpp with")
    exe = str(tmp_path / "rig_stream_guards")
    cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "event_flow_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "rig_stream_guards.cpp"), os.path.join(ROOT, "event_flow_amd", "csrc", "evf_stream.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
    assert "all guards answered EVF_EINVAL before any launch" in ran.stdout
