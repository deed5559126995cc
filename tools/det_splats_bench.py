"""Deterministic against default voxel binning and bilinear IWE at the spec shape (8 x 15 k events, 128 x 128), in one process:
python tools/det_splats_bench.py.  Per entry-point call, HIP-event brackets (_lib.profile_start), 3 warm-up calls and the median of
20 per block, the two modes alternated over two blocks each."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from event_flow_amd import _lib, synthetic
from event_flow_amd.dataloader.encodings import encode_event_list
from event_flow_amd.utils.iwe import compute_pol_iwe
B, n, H, W, nb, dev = 8, 15000, 128, 128, 5, "cuda:0"
g = np.random.default_rng(1)
ev = torch.from_numpy(synthetic.event_list_batch(B, n, H, W, 4242)).to(dev)
flow = torch.from_numpy(g.uniform(-0.1, 0.1, size=(B, 2, H, W)).astype(np.float32)).to(dev)
pol = torch.stack([(ev[:, :, 3] > 0).float(), (ev[:, :, 3] < 0).float()], 2).contiguous()
WORK = {"compute_pol_iwe(round_idx=False)": (lambda: compute_pol_iwe(flow, ev, (H, W), pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=128, round_idx=False),
                                             "evf_iwe_splat"),
        f"encode_event_list(voxel, nb={nb})": (lambda: encode_event_list(ev, nb, (H, W)), "evf_encode_events")}
before = _lib.deterministic()
for what, (run, name) in WORK.items():
    med = {False: [], True: []}
    for block in range(4):
        on = bool(block & 1)
        _lib.set_deterministic(on)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        entry = name + ("_det" if on else "")
        _lib.profile_start([entry])
        for _ in range(20):
            run()
        med[on].append(float(np.median(_lib.profile_stop()[(entry, "")])) * 1e3)
    off, on = float(np.mean(med[False])), float(np.mean(med[True]))
    print(f"{what}: default {off:.1f} us {['%.1f' % v for v in med[False]]}  deterministic {on:.1f} us {['%.1f' % v for v in med[True]]}  "
          f"ratio {on / off:.2f}  (launch floor {_lib.last_tiny_kernel_ms * 1e3:.1f} us)")
_lib.set_deterministic(before)
