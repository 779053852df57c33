"""``get_feature(x)`` of the bare backbones (the reference's ``model.get_feature``, models/c3d.py:111, resnet.py:203,
s3dg.py:151, r2plus1d_vcop.py:218) on the HIP kernels: the backbone's plan through engine.run_forward on the module's own packed
weights.  Used by retrieval.py on the model ModelFactory.build() returns.

Forward only.  ``module.training`` picks the BatchNorm mode as in the fine-tune path (split_wrapper._FinetuneFn): eval mode runs
on the running statistics, train mode on the batch statistics and moves the running buffers (and num_batches_tracked)."""
import torch
from torch import Tensor, nn

from .. import ops as _ops
from ..engine import INPUT_CHANNEL_PAD, PackedWeights, run_forward


def _to_ndhwc(x: Tensor) -> Tensor:
    be = _ops.backend()
    B = x.shape[0]
    src = torch.arange(B, dtype=torch.int32, device=x.device)
    step = torch.ones(B, dtype=torch.int32, device=x.device)
    return be.clip_gather(x.contiguous(), src, step, x.shape[2], max(x.shape[1], INPUT_CHANNEL_PAD))


def feature_ndhwc(module: nn.Module, x: Tensor) -> Tensor:
    """x: NCDHW (B, 3, T, H, W) on the device -> the backbone's feature map, NDHWC (B, T', H', W', C)."""
    params = list(module.parameters())
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        raise RuntimeError("get_feature is forward only (no autograd): call it under torch.no_grad(), as retrieval does")
    state = module.__dict__
    if "_feature_plan" not in state:
        state["_feature_plan"] = module.plan()
        state["_feature_packed"] = PackedWeights()
    # the weights may have been edited in place (a checkpoint load, an optimizer step) since the last call: re-pack when their
    # version counters moved
    ver = sum(p._version for p in params)
    if ver != state.get("_feature_version"):
        state["_feature_packed"].invalidate()
        state["_feature_version"] = ver
    training = module.training
    feat, _ = run_forward(state["_feature_plan"], _to_ndhwc(x), state["_feature_packed"], False, training=training)
    if training:
        for mod in module.modules():
            if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                mod.num_batches_tracked += 1
    return feat


def get_feature(module: nn.Module, x: Tensor) -> Tensor:
    """NCDHW in, NCDHW out (e.g. (B, 512, 1, 4, 4) for C3D at 16 x 112^2): a channels-first view of the NDHWC map."""
    return feature_ndhwc(module, x).permute(0, 4, 1, 2, 3)


class FeatureMixin:
    """Gives a backbone with a ``plan()`` the reference's ``get_feature``."""

    def get_feature(self, x: Tensor) -> Tensor:
        return get_feature(self, x)
