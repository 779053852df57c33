"""Backbone registry — same entry point and arch names as /root/reference/models/__init__.py:16-75."""
from typing import Callable

from torch import nn


def get_model_class(**kwargs) -> Callable[[int], nn.Module]:
    """``model_class(num_classes=N)`` factory for ``cfg['model']``; raises ValueError for unknown archs
    (models/__init__.py:73)."""
    arch = kwargs.get("arch")
    if arch == "c3d":
        from .c3d import C3D
        return C3D
    if arch in ("resnet18", "resnet34", "resnet50"):
        from . import resnet
        return getattr(resnet, arch)
    if arch == "s3dg":
        from .s3dg import S3D_G
        return S3D_G
    if arch == "r2plus1d-vcop":
        from .r2plus1d_vcop import R2Plus1DNet
        return lambda num_classes=128: R2Plus1DNet((1, 1, 1, 1), with_classifier=True, num_classes=num_classes)
    raise ValueError(f'Unknown model architecture "{arch}"')


class ModelFactory:
    """Downstream (fine-tune) model factory — same entry points as /root/reference/models/__init__.py:76-143.
    ``cfg`` is the resolved config (dict or pyhocon ConfigTree): keys ``model.arch``, ``dataset.num_classes``, ``only_train_fc``
    and — this project's own, the reference has no such switch — ``freeze_bn`` / ``freeze_bn_affine``."""

    def __init__(self, cfg):
        self.cfg = cfg

    def _get(self, dotted, default=None):
        node = self.cfg
        for part in dotted.split("."):
            if not hasattr(node, "get") or part not in node:
                return default
            node = node[part]
        return node

    def _post_process_model(self, model: nn.Module):
        """``only_train_fc``: freeze everything but the classifier and keep the backbone in eval mode (:82-104).
        ``freeze_bn`` (default false): fine-tune with frozen BatchNorm — ``train()`` keeps the encoder in eval mode (running
        statistics, buffers never move) and lets the classifier follow ``mode``; ``requires_grad`` is left alone, so every
        backbone parameter still trains.  With ``freeze_bn_affine`` (default false) the encoder's BatchNorm weight / bias are
        frozen as well.  ``only_train_fc`` wins if both are set."""
        if self._get("only_train_fc", False):
            for param in model.parameters():
                param.requires_grad = False
            fc_module = next((getattr(model, n) for n in ("fc", "new_fc") if hasattr(model, n)), None)
            if fc_module is None:
                raise Exception('"only_train_fc" specified, but no fc layer found')
            for param in fc_module.parameters():
                param.requires_grad = True
            orig_train = model.train

            def override_train(mode=True):
                orig_train(mode=False)
                fc_module.train(mode)

            model.train = override_train
        elif self._get("freeze_bn", False):
            encoder = getattr(model, "encoder", None)
            if encoder is None:
                raise Exception('"freeze_bn" specified, but the model has no encoder (use the multitask wrapper)')
            if self._get("freeze_bn_affine", False):
                for mod in encoder.modules():
                    if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                        for param in (mod.weight, mod.bias):
                            if param is not None:
                                param.requires_grad = False
            orig_train_bn = model.train

            def override_train_bn(mode=True):
                orig_train_bn(mode)
                encoder.eval()
                return model

            model.train = override_train_bn
            model.bn_frozen = True
        return model

    def build(self, local_rank: int) -> nn.Module:
        """The bare backbone ``get_model_class(**cfg.model)(num_classes=...)`` on cuda:local_rank (:108-123), wrapped like
        build_multitask_wrapper: DistributedDataParallel under a process group of more than one rank, else the pass-through
        holder.  Retrieval calls ``model.module.get_feature(clip)`` on it."""
        import torch
        import torch.distributed as dist
        model_cfg = dict(self._get("model"))
        model = get_model_class(**model_cfg)(num_classes=int(self._get("dataset.num_classes")))
        model = self._post_process_model(model)
        model = model.to(torch.device("cuda", local_rank))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return nn.parallel.DistributedDataParallel(model, device_ids=[local_rank])
        return _SingleProcess(model)

    def build_multitask_wrapper(self, local_rank: int) -> nn.Module:
        """MultiTaskWrapper(finetune=True) on cuda:local_rank, wrapped in DistributedDataParallel when a process group is up
        (:125-143); with a single process it is wrapped in a pass-through holder so that ``model.module`` exists either way."""
        import torch
        import torch.distributed as dist
        from ..moco.split_wrapper import MultiTaskWrapper
        model_cfg = dict(self._get("model"))
        model = MultiTaskWrapper(get_model_class(**model_cfg), num_classes=int(self._get("dataset.num_classes")), finetune=True)
        model = self._post_process_model(model)
        # (finetune.py:160-161: cuda:local_rank, the CPU only where there is no GPU -- there the model runs on the checker
        #  backend the CPU tests install and on nothing else: HipOps refuses host tensors)
        model = model.to(torch.device("cuda", local_rank) if torch.cuda.is_available() else torch.device("cpu"))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return nn.parallel.DistributedDataParallel(model, device_ids=[local_rank], find_unused_parameters=True)
        return _SingleProcess(model)


class _SingleProcess(nn.Module):
    """What DistributedDataParallel is to one rank: forwards to ``.module`` (checkpoints are saved from ``.module``)."""

    def __init__(self, module: nn.Module):
        super().__init__()
        self.module = module

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def train(self, mode: bool = True):
        self.training = mode
        self.module.train(mode)
        return self
