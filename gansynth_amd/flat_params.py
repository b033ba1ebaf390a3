"""The trainable variables of one network in one flat fp32 buffer: one fused Adam launch, one all-reduce payload."""
from collections import OrderedDict

import torch

_PAD = 64  # floats; keeps every parameter view 256-byte aligned inside the flat buffer


class _FlatParams(object):
    """All trainable variables of one scope re-homed into one flat fp32 buffer (+grad, m, v)."""

    def __init__(self, named_params):
        self.named = OrderedDict(named_params)
        sizes = [p.numel() for p in self.named.values()]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += (n + _PAD - 1) // _PAD * _PAD
        dev = next(iter(self.named.values())).device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.numel = sum(sizes)
        for (name, p), off, n in zip(self.named.items(), offs, sizes):
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view(p.shape)
            p.grad = self.grad[off:off + n].view(p.shape)
        self.t = 0
        self.grad_clean = True   # the flat gradient is all zeros (fresh buffer / cleared by the optimizer step)
        self.buckets = [(0, total)]
        self._offsets = list(zip(offs, sizes, self.named.keys()))
        self.avg = None          # the exponential moving average of `flat` (enable_average: the generator's only)

    def enable_average(self):
        """Allocate the shadow buffer of tf.train.ExponentialMovingAverage: a clone of `flat` as it is now (a fresh TF shadow variable starts
        at its variable's value), same layout -- the padding gaps are zero in both and stay zero under the update (0 - (0 - 0) * x)."""
        if self.avg is None:
            self.avg = self.flat.detach().clone()
        return self.avg

    def avg_view(self, name):
        """The average of variable `name`, shaped like it (a view into `avg`)."""
        p = self.named[name]
        off = (p.data.data_ptr() - self.flat.data_ptr()) // 4
        return self.avg[off:off + p.numel()].view(p.shape)

    def make_buckets(self, max_floats, reverse=False):
        """Split the flat buffer into contiguous ranges of whole tensors, each <= max_floats unless a single tensor is larger
        (the generator's 4.2 M-element dense weight gets a bucket of its own), ordered as the backward pass completes them:
        `reverse` for the generator (its backward ends at the first variables), natural order for the discriminator."""
        total = self.flat.numel()
        starts = [o for o, _, _ in self._offsets] + [total]
        buckets, a = [], 0
        for i in range(len(self._offsets)):
            nxt = starts[i + 1]
            if nxt - a > max_floats and starts[i] > a:      # closing before this tensor keeps the bucket under the limit
                buckets.append((a, starts[i]))
                a = starts[i]
            if nxt - a >= max_floats:
                buckets.append((a, nxt))
                a = nxt
        if a < total:
            buckets.append((a, total))
        self.buckets = buckets[::-1] if reverse else buckets
        return self.buckets

    def bucket_of(self, ptr):
        """Index (in completion order) of the bucket holding the gradient element at device address `ptr`, or None."""
        off = (ptr - self.grad.data_ptr()) // 4
        if 0 <= off < self.grad.numel():
            for i, (a, b) in enumerate(self.buckets):
                if a <= off < b:
                    return i
        return None

    def requires_grad_(self, flag):
        for p in self.named.values():
            p.requires_grad_(flag)

    def zero_grad(self):
        self.grad_clean = False
        self.begin_run()

    def begin_run(self):
        """Gradients of a run are accumulated in place from zero.  The previous optimizer step may have left the buffer cleared
        (gs_adam_tf_step_zero_grad, `grad_clean`): then there is no fill pass."""
        if not self.grad_clean:
            self.grad.zero_()
        self.grad_clean = False   # (about to be accumulated into)
        for p in self.named.values():
            if p.grad is None:
                raise RuntimeError("parameter lost its flat gradient view")
