"""Host reference of evf_activity_at (csrc/evf_activity.hip): exact integer counts with numpy alone -- `count_nonzero` of float32
(torch.ne(0)'s rule: -0.0 is zero; NaN, +-inf and every denormal are not) and the set bits of 32-bit words.  Shared by
tests/test_host_activity.py and tests/test_gpu_activity.py.  Not a test module itself."""

import numpy as np

FLOAT, WORDS = 0, 1
SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099)
# what a float source must hold: both zeros, NaN, both infinities, the smallest denormals of both signs, ordinary values
FLOAT_SPECIALS = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -2.5, 3e-39, 0.0, 7.0], dtype=np.float32)
WORD_SPECIALS = np.array([0, 0xFFFFFFFF, 0x80000000, 1, 0x00010000, 0, 0xAAAAAAAA], dtype=np.uint32)


def count_float(a):
    """Elements of a float32 array with x != 0, per leading index: int64 [B]."""
    a = np.asarray(a)
    assert a.dtype == np.float32
    return np.count_nonzero(a.reshape(a.shape[0], -1), axis=1).astype(np.int64)


def popcount(a):
    """Set bits of a 32-bit integer array, per leading index: int64 [B]."""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.uint32, np.int32)
    rows = a.reshape(a.shape[0], -1).view(np.uint8)
    return np.unpackbits(rows, axis=1).sum(axis=1, dtype=np.int64)


def counts(sources):
    """sources: [(kind, array [B, n])] -> int64 [nsrc, B], the row evf_activity_at stores (parts added)."""
    return np.stack([count_float(a) if kind == FLOAT else popcount(a) for kind, a in sources])


def float_data(rng, B, n, zeros=0.5):
    """float32 [B, n]: the specials first (as far as n reaches, rotated per sample), then ordinary values, about `zeros` of
    them zero (of either sign)."""
    out = rng.standard_normal((B, n)).astype(np.float32)
    hit = rng.random((B, n)) < zeros
    out[hit] = np.where(rng.random(int(hit.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    for b in range(B):
        sp = np.roll(FLOAT_SPECIALS, b)[:n]
        out[b, :sp.size] = sp
    return out


def word_data(rng, B, n):
    """uint32 [B, n]: the specials first (rotated per sample), then random words."""
    out = rng.integers(0, 1 << 32, size=(B, n), dtype=np.uint64).astype(np.uint32)
    for b in range(B):
        sp = np.roll(WORD_SPECIALS, b)[:n]
        out[b, :sp.size] = sp
    return out
