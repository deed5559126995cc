"""Device buffers between sentinel guards, shared by the GPU tests that call kernels through the C ABI
(tests/test_gpu_step_tail.py, tests/test_gpu_neuron_gen.py).  Not a test module itself."""

import numpy as np
import torch

DEV = "cuda:0"
GUARD = 64
SENTINEL = -724625.0  # (exact in fp32; no kernel under test produces it)
F32 = np.float32


class Bufs:
    """Device buffers between guards.  new(data) -> a Buf whose .t is the [n] payload view of a [64 (+ shift) | n | 64] tensor
    filled with the sentinel; check() asserts that no guard element of any buffer changed."""

    class Buf:
        def __init__(self, data, shift):
            data = np.ascontiguousarray(data, F32)
            self.shape, n = data.shape, data.size
            self.lo = GUARD + shift
            self.full = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
            self.t = self.full[self.lo:self.lo + n]
            self.set(data)
            assert self.ptr % 16 == 4 * (shift % 4)

        @property
        def ptr(self):
            return self.t.data_ptr()

        def set(self, data):
            self.t.copy_(torch.from_numpy(np.array(data, F32).reshape(-1)))  # (a copy: the shared inputs are read-only)

        def get(self):
            return self.t.cpu().numpy().reshape(self.shape)

        def guards_intact(self):
            return (self.full[:self.lo] == SENTINEL).all() & (self.full[self.lo + self.t.numel():] == SENTINEL).all()

    def __init__(self):
        self.all = []

    def new(self, data, shift=0):
        b = Bufs.Buf(data, shift)
        self.all.append(b)
        return b

    def check(self):
        assert bool(torch.stack([b.guards_intact() for b in self.all]).all()), "a kernel wrote into a guard region"
