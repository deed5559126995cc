"""float64 / numpy restatement of the training log's rows (csrc/evf_train_log.hip), shared by tests/test_gpu_train_log.py and
tests/test_gpu_train_monitor.py.  Not a test module itself."""

import numpy as np

F32 = np.float32
MEAN_RTOL = 2.0 ** -23  # one float32 rounding of the result (2^-24) + a float64 sum over n <= 2^25 terms (2^-28), factor-2 margin


def clip_head(total, max_norm):
    """(grad_norm, clip_coef) in float32 arithmetic from the squared norm the step kernel left: k_clip_adam_fused's expression,
    coef = fminf(1, max_norm / (sqrtf(total) + 1e-6f)), 1 when max_norm <= 0."""
    total = F32(total)
    with np.errstate(all="ignore"):
        norm = np.sqrt(total, dtype=F32)
        coef = F32(1.0)
        if max_norm > 0:
            coef = np.fmin(F32(1.0), F32(max_norm) / (norm + F32(1e-6)))
    return F32(norm), F32(coef)


def grad_means(g, segments, coef):
    """float64 mean of |g * coef| per segment [(offset, n)]: coef * sum|g| / n."""
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        return [float(np.float64(coef) * np.abs(g[o:o + n]).sum() / n) for o, n in segments]


def get_grads_ref(g, segments, coef):
    """The host `get_grads` on the clone scaled by the logged coefficient, in float32 like torch: per segment
    (mean in float64, min, max of |fl32(g * coef)|)."""
    g = np.asarray(g, F32)
    out = []
    with np.errstate(all="ignore"):
        for o, n in segments:
            a = np.abs(g[o:o + n] * F32(coef))
            out.append((float(np.float64(coef) * np.abs(g[o:o + n].astype(np.float64)).sum() / n), F32(a.min()), F32(a.max())))
    return out


def bit_count(words):
    """Set bits of an int32 array, through np.unpackbits."""
    return int(np.unpackbits(np.ascontiguousarray(words, np.int32).view(np.uint8)).sum())


def rate(count, total):
    return F32(np.float64(count) / np.float64(total))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)
