"""What the tools/time_*.py A/B timers share: the event-bracketed call loop, the operation counter of the tensor-library side and the
HBM copy rate the byte floors are quoted against."""
import torch
from torch.utils._python_dispatch import TorchDispatchMode

HBM_BYTES_PER_S = 6.29e12                                    # the measured HBM copy rate of the MI355X
VIEW_OPS = ("view", "reshape", "slice", "select", "unsqueeze", "squeeze", "expand", "transpose", "permute", "alias", "detach", "t.",
            "unbind", "as_strided", "_unsafe_view", "unflatten", "size", "stride", "is_", "numel", "dim", "lift_fresh", "split")


def timed(fn, calls):
    """ms per call of `fn` over `calls` back-to-back calls, between two device events (the caller warms `fn` first)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if not any(v in name for v in VIEW_OPS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_ops(fn):
    """ATen operations one call of `fn` dispatches that run on the device (views and metadata operations excluded)."""
    with OpCounter() as c:
        fn()
    return c.n
