"""TEST-ONLY: the torch checker backend (tests/cpu_ops.py) plus the eval-mode BatchNorm backward, restated in plain torch.

The plain CpuOps stays without the op on purpose: a backend that lacks it must keep raising the engine's RuntimeError
(tests/test_finetune_frozen_bn_cpu.py)."""
import torch
import torch.nn.functional as F

from cpu_ops import CpuOps, _ncdhw, _ndhwc
from rspnet_amd.ops import PoolGeom


class CpuOpsEval(CpuOps):
    name = "cpu-checker-eval"

    @torch.enable_grad()
    def bn_eval_act_pool_bwd(self, pg: PoolGeom, y, residual, dout, mean_invstd, scale_shift, relu, want_dres, dgamma_out, dbeta_out,
                             dy_out=None):
        C = y.shape[-1]
        z = self._act(pg, y, scale_shift, residual, relu).detach().requires_grad_(True)
        a = F.relu(z) if relu else z
        if pg.k != (1, 1, 1) or pg.s != (1, 1, 1):
            a = _ndhwc(F.max_pool3d(_ncdhw(a), pg.k, pg.s, pg.p))
        (dz,) = torch.autograd.grad(a, z, dout)
        Cv = C
        for v in (dgamma_out, dbeta_out):
            if v is not None:
                Cv = v.shape[0]
        scale = scale_shift[0].clone()
        scale[Cv:] = 0                                   # padding channels: dy = 0
        dy = dz * scale
        if dgamma_out is not None:
            xhat = (y - mean_invstd[0]) * mean_invstd[1]
            dgamma_out.copy_((dz.double() * xhat.double()).sum(dim=(0, 1, 2, 3)).float()[:Cv])
        if dbeta_out is not None:
            dbeta_out.copy_(dz.double().sum(dim=(0, 1, 2, 3)).float()[:Cv])
        dres = dz.contiguous() if want_dres else None
        if dy_out is not None:
            dy_out.copy_(dy)
            return dy_out, dres
        return dy.contiguous(), dres
