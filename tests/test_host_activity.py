"""activity.py without a device: fractions from hand-made counts, the CSV's header and bytes, the ring and drain arithmetic, the
refusals (each names its alternative), the row arithmetic row * P + p, the numpy reference the GPU tests compare against, and
the launcher's guards as a sanitized stand-alone program."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import activity_ref as ref

from event_flow_amd import _lib
from event_flow_amd import activity as A
from event_flow_amd.models.model import LIFFireNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIF_NEURON = {"leak": [-4.0, 0.1], "thresh": [0.8, 0.1], "learn_leak": True, "learn_thresh": True, "hard_reset": True}


def _model_cfg(width=32):
    return {"num_bins": 2, "base_num_channels": width, "kernel_size": 3, "encoding": "cnt", "norm_input": False,
            "mask_output": True, "activations": ["arctanspike", "arctanspike"], "spiking_neuron": dict(LIF_NEURON)}


def test_layers_are_the_names_of_log_true():
    assert A.LAYERS == ("0:input", "1:head", "2:G1", "3:R1a", "4:R1b", "5:G2", "6:R2a", "7:R2b", "8:pred")
    assert A.KINDS == (0, 1, 1, 1, 1, 1, 1, 1, 0) and (A.ACT_FLOAT, A.ACT_WORDS) == (ref.FLOAT, ref.WORDS)
    assert A.layer_bits(2, 3, 5) == [30, 480, 480, 480, 480, 480, 480, 480, 30]
    assert A.layer_bits(5, 4, 4) == [80] + [512] * 7 + [32]


def test_fractions_from_hand_made_counts():
    bits = A.layer_bits(2, 4, 4)  # 32, 512 x 7, 32
    counts = np.zeros((2, 9, 3), dtype=np.int64)
    counts[0, 0] = [32, 0, 16]
    counts[0, 1] = [1, 2, 3]
    counts[0, 8] = [0, 0, 1]
    counts[1, 7] = [512, 512, 512]
    batch, slots = A.fractions(counts, bits)
    assert batch.dtype == slots.dtype == np.float64 and batch.shape == (2, 9) and slots.shape == (2, 9, 3)
    assert batch[0, 0] == 48 / 96 and batch[0, 1] == 6 / 1536 and batch[0, 8] == 1 / 96 and batch[1, 7] == 1.0
    assert slots[0, 0].tolist() == [1.0, 0.0, 0.5] and slots[0, 1].tolist() == [1 / 512, 2 / 512, 3 / 512]
    assert batch[1, :7].tolist() == [0.0] * 7 and slots[1, 7].tolist() == [1.0] * 3
    # the batch-wide fraction is the mean of the slots' fractions only because every slot has the same number of bits
    assert np.array_equal(batch, slots.mean(axis=2))
    empty_b, empty_s = A.fractions(np.zeros((0, 9, 3), dtype=np.int64), bits)
    assert empty_b.shape == (0, 9) and empty_s.shape == (0, 9, 3)
    with pytest.raises(_lib.EvflowError, match="outside 0"):
        A.fractions(counts + 1, bits)  # 513 > 512
    with pytest.raises(_lib.EvflowError, match="expected"):
        A.fractions(np.zeros((2, 8, 3), dtype=np.int64), bits)


def test_row_arithmetic():
    assert [A.pass_row(r, 3, p) for r in (0, 1, 5) for p in range(3)] == [0, 1, 2, 3, 4, 5, 15, 16, 17]
    assert A.pass_row(7, 1, 0) == 7
    assert all(A.pass_row(-1, P, p) < 0 for P in (1, 3, 4) for p in range(P))  # a row word of -1 skips every pass
    for P, p in ((3, 3), (3, -1), (0, 0)):
        with pytest.raises(_lib.EvflowError):
            A.pass_row(0, P, p)


def test_ring_and_drain_arithmetic():
    ring = A.Ring(4)
    assert ring.pending == 0 and not ring.full and ring.take() == []
    rows = []
    for _ in range(4):
        rows.append(ring.next_row())
        ring.advance()
    assert rows == [0, 1, 2, 3] and ring.full and ring.pending == 4
    with pytest.raises(_lib.EvflowError, match="drain"):
        ring.next_row()
    assert ring.take() == [0, 1, 2, 3] and ring.pending == 0 and not ring.full
    for _ in range(3):
        rows.append(ring.next_row())
        ring.advance()
    assert rows[4:] == [0, 1, 2] and ring.take() == [0, 1, 2]
    ring.advance(3)  # a stepper's window of three passes through its own row word
    assert ring.pending == 3 and ring.take() == [3, 0, 1] and ring.steps == 10
    ring.next_row(ahead=4)
    with pytest.raises(_lib.EvflowError, match="drain"):
        ring.next_row(ahead=5)
    ring.advance(5)
    with pytest.raises(_lib.EvflowError, match="overwrote"):
        ring.take()
    with pytest.raises(_lib.EvflowError, match="at least one row"):
        A.Ring(0)


def _lines(path):
    with open(path, "rb") as f:
        return f.read().decode().split("\r\n")


def test_csv_bytes_b1(tmp_path):
    out = A.ActivityCsv(str(tmp_path / "a"))
    batch = np.array([[0.5, 1 / 3, 0, 0, 0, 0, 0, 1.0, 0.25], [0, 0, 0, 0.1, 0, 0, 0, 0, 0]])
    out.write(batch, batch[:, :, None], [False, True])
    out.write(batch[:1], batch[:1, :, None], [False])  # appended: no second header, the pass index goes on
    lines = _lines(tmp_path / "a" / "activity.csv")
    assert lines[0] == "pass,new_seq,0:input,1:head,2:G1,3:R1a,4:R1b,5:G2,6:R2a,7:R2b,8:pred"
    assert lines[1] == "0,1,0.5,0.333333343,0,0,0,0,0,1,0.25"  # %.9g of the float32 rounding; the first pass starts a sequence
    assert lines[2] == "1,1,0,0,0,0.100000001,0,0,0,0,0"
    assert lines[3] == "2,0,0.5,0.333333343,0,0,0,0,0,1,0.25"
    assert lines[4:] == [""]


def test_csv_bytes_b3(tmp_path):
    out = A.ActivityCsv(str(tmp_path))
    counts = np.zeros((1, 9, 3), dtype=np.int64)
    counts[0, 1] = [1, 2, 3]
    counts[0, 8] = [32, 0, 0]
    batch, slots = A.fractions(counts, A.layer_bits(2, 4, 4))
    out.write(batch, slots, [False])
    lines = _lines(tmp_path / "activity.csv")
    assert lines[0].split(",") == ["pass", "new_seq"] + list(A.LAYERS) + [f"b{k}/{layer}" for k in range(3) for layer in A.LAYERS]
    assert lines[1] == ("0,1,0,0.00390625,0,0,0,0,0,0,0.333333343"
                        ",0,0.001953125,0,0,0,0,0,0,1"
                        ",0,0.00390625,0,0,0,0,0,0,0"
                        ",0,0.005859375,0,0,0,0,0,0,0")
    with pytest.raises(_lib.EvflowError, match="disagree"):
        out.write(batch, slots, [False, False])
    # a path that reports batch-wide fractions only keeps the columns, empty
    host = A.ActivityCsv(str(tmp_path / "host"), B=3)
    host.write(batch, None, [False])
    assert _lines(tmp_path / "host" / "activity.csv")[1] == "0,1,0,0.00390625,0,0,0,0,0,0,0.333333343" + "," * 27


def test_report_means_and_files(tmp_path):
    counts = np.zeros((3, 9, 2), dtype=np.int64)
    counts[:, 1, 0] = [512, 256, 0]
    counts[:, 1, 1] = [0, 0, 128]
    batch, slots = A.fractions(counts, A.layer_bits(2, 4, 4))
    rep = A.Report(str(tmp_path), 2, per_sequence=True)
    rep.add(batch[:2], slots[:2], [True, False], [["a", "b"], ["a", "c"]])
    rep.add(batch[2:], slots[2:], [False], [["c", "c"]])
    out = rep.into({"per_sequence": {"a": {"FWL": 1.0, "it": 2}}})
    assert out["activity"]["1:head"] == (0.5 + 0.25 + 0.125) / 3 and out["activity"]["0:input"] == 0.0
    assert set(out["activity"]) == set(A.LAYERS)
    assert out["per_sequence"]["a"] == {"FWL": 1.0, "it": 2, "activity": {**{l: 0.0 for l in A.LAYERS}, "1:head": 0.75}}
    assert out["per_sequence"]["b"]["activity"]["1:head"] == 0.0
    assert out["per_sequence"]["c"]["activity"]["1:head"] == (0.0 + 0.0 + 0.25) / 3
    assert len(_lines(tmp_path / "activity.csv")) == 5
    quiet = A.Report(None, 2)
    quiet.add(batch, slots, [True, False, False])
    assert quiet.into({}) == {"activity": out["activity"]}


class EVFlowNet:  # stands for the EVFlowNet family: forward reports "activity": None, there is no compute_path
    pass


def test_refusals_name_the_alternative(monkeypatch):
    fused, general = LIFFireNet(_model_cfg(32)), LIFFireNet(_model_cfg(16))
    assert fused.compute_path[0] == "fused" and general.compute_path[0] == "general"
    assert A.refusal(fused) is None and A.path(fused) == "device"
    why = A.refusal(general)
    assert A.path(general) == "host" and "general path" in why and "model(..., log=True)" in why and "nine reads per pass" in why
    why = A.refusal(EVFlowNet())
    assert A.path(EVFlowNet()) is None and "EVFlowNet" in why and '"activity": None' in why and "FireNet" in why and "drop --activity" in why
    with pytest.raises(_lib.EvflowError, match="general path"):
        A.ActivityLog(general, 1)
    with pytest.raises(_lib.EvflowError, match="activity"):
        A.ActivityLog(EVFlowNet(), 1)
    with pytest.raises(_lib.EvflowError, match="at least one"):
        A.ActivityLog(fused, 0)
    with pytest.raises(_lib.EvflowError, match="at least one row"):
        A.ActivityLog(fused, 1, rows=0)
    monkeypatch.setenv("WORLD_SIZE", "2")
    why = A.refusal(fused)
    assert A.path(fused) is None and "WORLD_SIZE" in why and "WORLD_SIZE=1" in why and "drop --activity" in why


def test_the_reference_on_hand_written_cases():
    f = np.array([[0.0, -0.0, np.nan, np.inf], [-np.inf, 1e-45, -1e-45, 2.0], [0.0, 0.0, -0.0, -0.0]], dtype=np.float32)
    assert ref.count_float(f).tolist() == [2, 4, 0]
    assert (f[1, 1] != 0) and f[1, 1].view(np.uint32) == 1  # 1e-45 IS the smallest denormal, not zero
    w = np.array([[0, 0xFFFFFFFF, 0x80000000], [1, 3, 0xF0F0F0F0], [0, 0, 0]], dtype=np.uint32)
    assert ref.popcount(w).tolist() == [33, 19, 0]
    assert ref.popcount(w.view(np.int32)).tolist() == [33, 19, 0]
    assert ref.counts([(ref.FLOAT, f), (ref.WORDS, w)]).tolist() == [[2, 4, 0], [33, 19, 0]]
    assert ref.count_float(f.reshape(3, 2, 2)).tolist() == [2, 4, 0]
    rng = np.random.default_rng(5)
    fd, wd = ref.float_data(rng, 3, 4099), ref.word_data(rng, 3, 4099)
    bits = fd.view(np.uint32)
    assert ref.count_float(fd).tolist() == [int(((bits[b] & 0x7FFFFFFF) != 0).sum()) for b in range(3)]
    assert ref.popcount(wd).tolist() == [sum(bin(int(v)).count("1") for v in wd[b]) for b in range(3)]
    for special in (np.float32(-0.0), np.float32(1e-45), np.float32(np.nan)):  # the specials are in every sample
        assert all((fd[b].view(np.uint32) == special.view(np.uint32)).any() for b in range(3))
    assert all((wd[b] == 0xFFFFFFFF).any() and (wd[b] == 0x80000000).any() for b in range(3))
    assert ref.float_data(rng, 3, 1).shape == (3, 1) and ref.word_data(rng, 3, 2).shape == (3, 2)


def test_launcher_guards_as_a_sanitized_stand_alone_program(tmp_path):
    """tools/activity_guards.cpp with csrc/evf_activity.hip, host code under AddressSanitizer and UBSan: every EVF_EINVAL case is
    answered before any launch (the program makes no accepted call, so it never launches)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc to build tools/activity_guards.cpp with")
    exe = str(tmp_path / "activity_guards")
    cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "event_flow_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "activity_guards.cpp"), os.path.join(ROOT, "event_flow_amd", "csrc", "evf_activity.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-3000:]
    assert "all guards answered EVF_EINVAL before any launch" in ran.stdout
