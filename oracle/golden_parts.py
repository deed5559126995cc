"""Fixtures stored as numbered parts  --  test infrastructure only.

The XLIF / ALIF FireNet reference runs (tools/gen_golden.py::g7_adaptive_firenet) hold the same arrays as the other g7 files but are
written as tests/golden/<name>.partNN.npz, every part below the 1 MiB a committed file may have.  `load_parts` gives them back as one
read-only mapping with the `.files` list of an opened .npz, so code written for `np.load` reads them unchanged.
"""

import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


class Parts(dict):
    @property
    def files(self):
        return list(self.keys())


def load_parts(name, root=GOLDEN):
    paths = sorted(glob.glob(os.path.join(root, name + ".part[0-9][0-9].npz")))
    if not paths:
        raise FileNotFoundError(os.path.join(root, name + ".part00.npz"))
    out = Parts()
    for i, path in enumerate(paths):
        if not path.endswith(f".part{i:02d}.npz"):
            raise FileNotFoundError(f"{name}: part {i:02d} is missing")
        with np.load(path) as g:
            for k in g.files:
                if k in out:
                    raise KeyError(f"{name}: {k} is in two parts")
                out[k] = g[k]
    return out


def adaptive_margin(g, layers):
    """min |v' - (t0 + t1 * trace')| over the passes, layers and elements of an XLIF / ALIF g7 fixture, from its stored arrays."""
    worst = np.inf
    for i in range(int(g["meta_P"])):
        for ln in layers:
            thr = np.maximum(g[f"param0_{ln}.t0"], np.float32(0.01))[None] + np.maximum(g[f"param0_{ln}.t1"], np.float32(0))[None] * g[f"p{i}_aux_{ln}"]
            worst = min(worst, float(np.abs(g[f"p{i}_v_{ln}"] - thr).min()))
    return worst
