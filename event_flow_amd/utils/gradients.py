"""`vis.store_grads` on the host -- counterpart of the reference's utils/gradients.py `get_grads`: mean, min and max of |grad| of
every parameter whose name contains "weight", read after `clip_grad_norm_` (train_flow.py:157-160).  The fused-optimizer steps,
whose gradient is consumed by the step kernel, log the same numbers on the device (event_flow_amd.monitor.TrainMonitor)."""


def get_grads(named_parameters):
    """-> {"<name>_mean" | "<name>_min" | "<name>_max": float} in named_parameters() order; parameters without a gradient are
    skipped.  One host read per tensor."""
    out = {}
    for name, p in named_parameters:
        if "weight" not in name or not p.requires_grad or p.grad is None:
            continue
        g = p.grad.detach().abs()
        mean, lo, hi = g.mean(), g.min(), g.max()
        out[f"{name}_mean"], out[f"{name}_min"], out[f"{name}_max"] = float(mean), float(lo), float(hi)
    return out
