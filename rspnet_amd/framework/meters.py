"""Running meters of an epoch (framework/meters/average.py) kept as ONE device struct, so that a HIP call can update all of them."""
import ctypes

import numpy as np
import torch
import torch.distributed as dist


class DeviceMeters:
    """N = len(KEYS) AverageMeters as ``val[N]`` fp32 | ``sum[N]`` fp32 | ``count[N]`` int32 in one uint8 device tensor, ``buf``: the
    layout of STRUCT, which a kernel updates on the device.  ``read`` is the only host synchronisation.  A subclass supplies NAMES,
    KEYS, FMTS (AverageMeter's name / fmt per entry) and STRUCT (the ctypes mirror of the C struct)."""

    NAMES = KEYS = FMTS = ()
    STRUCT = None

    def __init__(self, device):
        n = len(self.KEYS)
        assert 12 * n == ctypes.sizeof(self.STRUCT)
        self.device = torch.device(device)
        self.buf = torch.zeros(12 * n, dtype=torch.uint8, device=self.device)
        self.val = self.buf[0:4 * n].view(torch.float32)
        self.sum = self.buf[4 * n:8 * n].view(torch.float32)
        self.count = self.buf[8 * n:12 * n].view(torch.int32)

    def reset(self):
        self.buf.zero_()

    @torch.no_grad()
    def update(self, values, n: int):
        """AverageMeter.update(v_i, n) for the first len(values) entries, in KEYS order, from torch ops -- the path of a backend
        without the HIP entry point, and of host tensors.  The other entries stay as they are."""
        v = torch.stack([x.detach().to(torch.float32).reshape(()) for x in values]).to(self.device)
        k = v.numel()
        self.val[:k] = v
        self.sum[:k] += v * n
        self.count[:k] += n

    def read(self):
        """{key: {val, avg, sum, count}}; avg = sum / count in fp32 (NaN while count is 0).  Synchronises."""
        n = len(self.KEYS)
        host = self.buf.cpu().numpy()
        val, total, count = host[:4 * n].view(np.float32), host[4 * n:8 * n].view(np.float32), host[8 * n:].view(np.int32)
        with np.errstate(divide="ignore", invalid="ignore"):
            avg = total / count.astype(np.float32)
        return {k: {"val": float(val[i]), "avg": float(avg[i]), "sum": float(total[i]), "count": int(count[i])}
                for i, k in enumerate(self.KEYS)}

    def sync_distributed(self):
        """All-reduce sum and count over the ranks (AverageMeter.sync_distributed); nothing to do on one rank."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            works = [dist.all_reduce(self.count, op=dist.ReduceOp.SUM, async_op=True),
                     dist.all_reduce(self.sum, op=dist.ReduceOp.SUM, async_op=True)]
            for w in works:
                w.wait()

    def pieces(self, stats=None):
        """['Loss {val:f} ({avg:f})', 'Acc@1 {val:6.2f} ({avg:6.2f})', ...] as AverageMeter.__str__ formats them."""
        stats = stats or self.read()
        return [("{name} {val" + fmt + "} ({avg" + fmt + "})").format(name=name, val=stats[k]["val"], avg=stats[k]["avg"])
                for name, k, fmt in zip(self.NAMES, self.KEYS, self.FMTS)]

    def __str__(self):
        return "\t".join(self.pieces())
