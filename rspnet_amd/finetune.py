"""Action-recognition fine-tuning around ``MultiTaskWrapper(finetune=True)`` -- the reference's finetune.py: multi-crop reshape +
logit averaging (finetune.py:44-61), the pretext-checkpoint loader with its prefix / blacklist rule (:273-310), the train / validate
steps (:95-116, :326-345), and the driver around them: ``FusedCrossEntropy`` + ``Meters`` (everything behind the logits of one
iteration, :101-143, as ONE HIP call, rsp_xent_metrics), ``Engine`` (:149-424: optimizer, the four LR schedules, epoch loop with the
tail cut, best-accuracy checkpoint) and ``python -m rspnet_amd.finetune`` (:426-502, final multi-crop validation included).

Not rebuilt: video decoding and the dataset classes (the loaders are any iterable of ``((clip,), target, *others)`` with ``__len__``,
``set_epoch``, ``num_valid_samples`` and ``.dataset``; ``SyntheticLabelledClips`` stands in), ``save_results`` of the final
validation, TensorBoard (per-epoch scalars go to ``scalars.jsonl``), ``model_type: '1stream'``.  One rank is the supported
configuration; the multi-rank path (DDP from the model factory, ``Meters.sync_distributed``) has never run on more than one GPU.

Accuracy ranks an exact tie of two logits in favour of the lower class index; ``torch.topk``, which the reference uses, leaves the
order of tied entries unspecified.  That is the one divergence."""
from __future__ import annotations

import argparse
import logging
import time
from pathlib import Path
from typing import Dict, Optional

import torch
import torch.distributed as dist
from torch import Tensor, nn

from . import _lib, fingerprint, ops
from .framework.arguments import add_driver_arguments, parse_driver_args
from .framework.driver import (append_scalars, finish_process_group, init_process_group, launch, load_config, load_states, save_run,
                               seed_everything, setup_logging)
from .framework.meters import DeviceMeters

logger = logging.getLogger(__name__)
BLACKLIST = ("fc.", "linear", "head", "new_fc", "fc8", "encoder_fuse")


def reshape_clip(clip: Tensor, n_crop: int) -> Tensor:
    """(B, C, n_crop*T, H, W) -> (B*n_crop, C, T, H, W), crops of one sample adjacent (finetune.py:44-52)."""
    if n_crop == 1:
        return clip
    B, C, TT, H, W = clip.shape
    T = TT // n_crop
    return clip.view(B, C, n_crop, T, H, W).permute(0, 2, 1, 3, 4, 5).reshape(B * n_crop, C, T, H, W)


def average_logits(logits: Tensor, n_crop: int) -> Tensor:
    """(B*n_crop, classes) -> (B, classes), mean over the crops of a sample (finetune.py:54-61)."""
    if n_crop == 1:
        return logits
    return logits.view(logits.shape[0] // n_crop, n_crop, -1).mean(dim=1)


def load_moco_checkpoint(model: nn.Module, checkpoint_path: str, device=None) -> "torch.nn.modules.module._IncompatibleKeys":
    """finetune.py:273-310: keep ``encoder_q.*`` of a pretext checkpoint (or ``module.*`` / bare keys of a third-party one),
    drop the classifier-like names, load non-strictly.  ``model`` is the unwrapped MultiTaskWrapper."""
    cp = torch.load(checkpoint_path, map_location=device, weights_only=False)
    if "model" in cp and "arch" in cp:
        state, prefix = cp["model"], "encoder_q."
    else:
        state = cp["state_dict"] if "state_dict" in cp else cp
        prefix = "module." if next(iter(state.keys())).startswith("module") else ""
    keep = {k[len(prefix):]: v for k, v in state.items()
            if k.startswith(prefix) and not any(k.startswith(f"{prefix}{b}") for b in BLACKLIST)}
    msg = model.load_state_dict(keep, strict=False)
    logger.warning("Missing keys: %s, Unexpected keys: %s", msg.missing_keys, msg.unexpected_keys)
    return msg


def train_step(model: nn.Module, criterion: nn.Module, optimizer: torch.optim.Optimizer, clip: Tensor, target: Tensor) -> Dict:
    """One optimisation step as finetune.py:326-338 runs it (n_crop = 1 in training)."""
    output = model(clip)
    loss = criterion(output, target)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return {"loss": loss.detach(), "output": output.detach()}


@torch.no_grad()
def validate_step(model: nn.Module, criterion: nn.Module, clip: Tensor, target: Tensor, n_crop: int = 1) -> Dict:
    """finetune.py:95-116 under ``model.eval()``: crops -> logits -> mean over crops -> loss."""
    output = average_logits(model(reshape_clip(clip, n_crop)), n_crop)
    return {"loss": criterion(output, target), "output": output}


# ---- meters and criterion (finetune.py:101-143 behind the logits) ----------------------------------------------------------
class Meters(DeviceMeters):
    """The three running meters of an epoch context (loss, Acc@1, Acc@5) over rsp_cls_meters; FusedCrossEntropy updates them on the
    device."""

    NAMES = ("Loss", "Acc@1", "Acc@5")
    KEYS = ("loss", "acc1", "acc5")
    FMTS = (":f", ":6.2f", ":6.2f")
    STRUCT = _lib.ClsMeters


def rank_of_target(output: Tensor, target: Tensor) -> Tensor:
    """rank(s) = #{c : out[s][c] > out[s][t]} + #{c < t : out[s][c] == out[s][t]} -- the tie rule of rsp_xent_metrics in torch ops."""
    vt = output.gather(1, target.view(-1, 1))
    cls = torch.arange(output.shape[1], device=output.device).view(1, -1)
    return ((output > vt) | ((output == vt) & (cls < target.view(-1, 1)))).sum(dim=1)


class _XentFn(torch.autograd.Function):
    """loss = rsp_xent_metrics(output); backward hands grad_out * dlogits to the producer of ``output``."""

    @staticmethod
    def forward(ctx, output: Tensor, target: Tensor, n_crop: int, valid: int, meters_buf, want_grad: bool):
        avg, loss, acc, dlogits = ops.backend().xent_metrics(output, target, n_crop=n_crop, valid=valid, want_grad=want_grad,
                                                             meters=meters_buf)
        ctx.dlogits = dlogits
        ctx.mark_non_differentiable(avg, acc)
        return loss.view(()), avg, acc

    @staticmethod
    def backward(ctx, grad_out, _gavg, _gacc):
        if ctx.dlogits is None:
            raise RuntimeError("FusedCrossEntropy: no gradient was computed (the forward ran without grad)")
        return grad_out * ctx.dlogits, None, None, None, None, None


class FusedCrossEntropy(nn.Module):
    """``average_logits`` + ``nn.CrossEntropyLoss()`` + ``accuracy(topk=(1, 5))`` over the first ``valid`` samples + the three
    ``AverageMeter.update`` calls of one iteration (finetune.py:104-141) as one HIP call.  Returns the scalar loss (mean over ALL
    samples, as finetune.py:105 takes it before the tail cut) as an autograd node; ``.output`` holds the crop-averaged logits,
    ``.acc`` the (acc1, acc5) device tensor of this call (acc5 is meaningful from 5 classes on).

    When the active op backend has no ``xent_metrics`` (the torch checker backend of the CPU tests) the same result is composed
    from torch ops."""

    def __init__(self):
        super().__init__()
        self.output = None
        self.acc = None

    def forward(self, output: Tensor, target: Tensor, n_crop: int = 1, valid: Optional[int] = None,
                meters: Optional[Meters] = None) -> Tensor:
        S = output.shape[0] // n_crop
        valid = S if valid is None else int(valid)
        be = ops.backend()
        if hasattr(be, "xent_metrics"):
            want_grad = torch.is_grad_enabled() and output.requires_grad
            loss, avg, acc = _XentFn.apply(output, target, n_crop, valid, None if meters is None else meters.buf, want_grad)
            self.output, self.acc = avg, acc
            return loss
        avg = average_logits(output, n_crop)
        loss = nn.functional.cross_entropy(avg, target)
        with torch.no_grad():
            out = avg.detach()
            self.output = out
            self.acc = None
            if valid > 0:
                rank = rank_of_target(out[:valid], target[:valid])
                ks = (1, 5) if out.shape[1] >= 5 else (1,)
                accs = [(rank < k).sum().to(torch.float32) * (100.0 / valid) for k in ks]     # classification.py:18-19
                self.acc = torch.stack(accs)
                if meters is not None:
                    meters.update([loss] + accs, valid)
        return loss


# ---- data stand-in ---------------------------------------------------------------------------------------------------------
class SyntheticLabelledClips:
    """Decode-free stand-in for the fine-tune loaders (datasets/classification DataLoaderFactoryV3): a fixed pool of device clips
    whose class is recoverable from the clip -- a per-class low-resolution spatio-temporal pattern (shared by the splits),
    upsampled to the clip size, plus N(0, 1) noise.  Yields ``((clip,), target)`` device batches.

    split 'train': n_crop = 1, shuffled per epoch (``set_epoch``), drop_last.  split 'val': the time axis holds n_crop * T frames,
    order fixed, every batch full -- the tail wraps around to the first samples, as the distributed sampler repeats samples, and
    ``num_valid_samples()`` says how many are real, so the consumer cuts the repeats (finetune.py:112-119)."""

    PATTERN_SEED = 20201
    POOL_BYTES = 1 << 30

    def __init__(self, split: str, num_samples: int, batch_size: int, num_classes: int, T: int, size: int, device, n_crop: int = 1,
                 seed: int = 0, amplitude: float = 1.0):
        assert split in ("train", "val") and num_samples >= 1
        self.split, self.num_samples, self.batch_size, self.seed = split, int(num_samples), int(batch_size), int(seed)
        self.device = torch.device(device)
        self.dataset = self
        frames = T * (n_crop if split == "val" else 1)
        g = torch.Generator().manual_seed(self.PATTERN_SEED)
        pattern = torch.randn(num_classes, 3, 2, 4, 4, generator=g).to(self.device)
        pool = max(1, min(self.num_samples, self.POOL_BYTES // (3 * frames * size * size * 4)))
        gs = torch.Generator().manual_seed(1000003 * (1 if split == "val" else 2) + self.seed)
        labels = torch.randint(0, num_classes, (self.num_samples,), generator=gs)
        labels[pool:] = labels[torch.arange(pool, self.num_samples) % pool]      # sample i shows pool clip i % pool
        self.labels = labels.to(self.device)
        gd = torch.Generator(device=self.device).manual_seed(gs.initial_seed() + 1) if self.device.type == "cuda" else gs
        self.pool = torch.empty(pool, 3, frames, size, size, device=self.device)
        for i in range(pool):
            c = int(labels[i])
            up = nn.functional.interpolate(pattern[c:c + 1], size=(frames, size, size), mode="nearest")[0]
            self.pool[i] = amplitude * up + torch.randn(3, frames, size, size, device=self.device, generator=gd)
        self._order = None
        self.set_epoch(0)

    def __len__(self):
        if self.split == "train":
            return self.num_samples // self.batch_size
        return (self.num_samples + self.batch_size - 1) // self.batch_size

    def num_valid_samples(self) -> int:
        return len(self) * self.batch_size if self.split == "train" else self.num_samples

    def set_epoch(self, epoch: int):
        """The epoch's sample order goes to the device once, here: iterating moves no host data."""
        n = len(self) * self.batch_size
        if self.split == "train":
            g = torch.Generator().manual_seed(self.seed + 7919 * int(epoch))
            order = torch.randperm(self.num_samples, generator=g)[:n]
        else:
            order = torch.arange(n) % self.num_samples
        self._order = order.to(self.device)

    def __iter__(self):
        B = self.batch_size
        for b in range(len(self)):
            idx = self._order[b * B:(b + 1) * B]
            yield (self.pool.index_select(0, idx % self.pool.shape[0]),), self.labels.index_select(0, idx)


# ---- engine (finetune.py:149-424) ------------------------------------------------------------------------------------------
def _get(cfg, dotted: str, default=None):
    node = cfg
    for part in dotted.split("."):
        if not hasattr(node, "get") or part not in node:
            return default
        node = node[part]
    return node


def _need(cfg, dotted: str):
    v = _get(cfg, dotted)
    if v is None:
        raise KeyError(f'config key "{dotted}" is required')
    return v


def build_scheduler(schedule_type: str, optimizer, cfg, num_epochs: int, learning_rate: float):
    """optimizer.schedule -> torch scheduler (finetune.py:210-235)."""
    sched = torch.optim.lr_scheduler
    if schedule_type == "plateau":
        return sched.ReduceLROnPlateau(optimizer=optimizer, mode="min", patience=int(_need(cfg, "optimizer.patience")))
    if schedule_type == "multi_step":
        return sched.MultiStepLR(optimizer=optimizer, milestones=list(_need(cfg, "optimizer.milestones")))
    if schedule_type == "cosine":
        return sched.CosineAnnealingLR(optimizer=optimizer, T_max=num_epochs, eta_min=learning_rate / 1000)
    if schedule_type == "none":
        return sched.LambdaLR(optimizer=optimizer, lr_lambda=_constant_one)
    raise ValueError(f'Unknown schedule type "{schedule_type}"')


def _constant_one(epoch):
    return 1


class Engine:
    def __init__(self, args, cfg: dict, local_rank: int, final_validate: bool = False, train_loader=None, validate_loader=None):
        from .models import ModelFactory
        self.args, self.cfg, self.local_rank, self.final_validate = args, cfg, local_rank, final_validate
        self.device = torch.device("cuda", local_rank) if torch.cuda.is_available() else torch.device("cpu")
        model_type = _need(cfg, "model_type")
        if model_type == "1stream":
            raise NotImplementedError("model_type '1stream' is not rebuilt: the bare backbones have no classifier backward here; "
                                      "use model_type 'multitask'")
        if model_type != "multitask":
            raise ValueError(f'Unrecognized model_type "{model_type}"')
        self.model = ModelFactory(cfg).build_multitask_wrapper(local_rank)      # (honours only_train_fc, freeze_bn, freeze_bn_affine)
        if getattr(self.model.module, "bn_frozen", False):
            logger.info("BatchNorm frozen: the encoder stays on its running statistics while it trains (freeze_bn)%s",
                        "; BatchNorm weight / bias frozen too (freeze_bn_affine)" if _get(cfg, "freeze_bn_affine", False) else "")
        self.n_crop = int(_need(cfg, "temporal_transforms.validate.final_n_crop" if final_validate
                                else "temporal_transforms.validate.n_crop"))
        self.criterion = FusedCrossEntropy()

        self.learning_rate = float(_need(cfg, "optimizer.lr"))
        optimizer_type = _get(cfg, "optimizer.type", "sgd")
        if optimizer_type == "sgd":
            self.optimizer = torch.optim.SGD(self.model.parameters(), lr=self.learning_rate,
                                             momentum=float(_need(cfg, "optimizer.momentum")),
                                             dampening=float(_need(cfg, "optimizer.dampening")),
                                             weight_decay=float(_need(cfg, "optimizer.weight_decay")),
                                             nesterov=bool(_need(cfg, "optimizer.nesterov")))
        elif optimizer_type == "adam":
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=self.learning_rate, eps=float(_need(cfg, "optimizer.eps")))
        else:
            raise ValueError(f"Unknown optimizer {optimizer_type})")
        self.num_epochs = int(_need(cfg, "num_epochs"))
        self.schedule_type = _need(cfg, "optimizer.schedule")
        self.scheduler = build_scheduler(self.schedule_type, self.optimizer, cfg, self.num_epochs, self.learning_rate)
        self.arch = _need(cfg, "model.arch")
        self.log_interval = int(_need(cfg, "log_interval"))

        self.train_loader = None
        if not final_validate:
            self.train_loader = train_loader if train_loader is not None else self._synthetic("train")
        self.validate_loader = validate_loader if validate_loader is not None else self._synthetic("val")

        self.best_acc1 = 0.
        self.current_epoch = 0
        self.train_stats = self.validate_stats = None
        logger.info("Engine: n_crop=%d", self.n_crop)
        from .framework.utils.checkpoint import CheckpointManager
        self.checkpoint_manager = CheckpointManager(args.experiment_dir, keep_interval=None)
        run_dir = getattr(args, "run_dir", None)
        self.scalars_path = None if run_dir is None or local_rank != 0 else Path(run_dir) / "scalars.jsonl"
        # opt-in (config key "fingerprint", e.g. -x '{"fingerprint": {"every": 50, "halt_on_nonfinite": true}}'): None otherwise
        self.fingerprints = fingerprint.StepFingerprints.from_config(cfg, run_dir, rank=local_rank)

    def _synthetic(self, split: str):
        cfg, a = self.cfg, self.args
        T, size = int(_need(cfg, "temporal_transforms.size")), int(_need(cfg, "spatial_transforms.size"))
        classes, seed = int(_need(cfg, "dataset.num_classes")), int(getattr(a, "seed", 0) or 0)
        if split == "train":
            B = int(_need(cfg, "batch_size"))
            return SyntheticLabelledClips("train", B * int(getattr(a, "steps_per_epoch", 100)), B, classes, T, size, self.device,
                                          seed=seed)
        B = int(_need(cfg, "final_validate.batch_size" if self.final_validate else "validate.batch_size"))
        return SyntheticLabelledClips("val", int(getattr(a, "val_samples", 100)), B, classes, T, size, self.device,
                                      n_crop=self.n_crop, seed=seed)

    # ---- checkpoints (finetune.py:259-310) ---------------------------------------------------------------------------
    def load_checkpoint(self, checkpoint_path):
        states = load_states(checkpoint_path, self.device, self.arch)
        logger.info("Loading checkpoint from %s", checkpoint_path)
        self.model.module.load_state_dict(states["model"])
        logger.info("Checkpoint loaded")
        self.optimizer.load_state_dict(states["optimizer"])
        self.scheduler.load_state_dict(states["scheduler"])
        self.current_epoch = states["epoch"]
        self.best_acc1 = states["best_acc1"]

    def load_moco_checkpoint(self, checkpoint_path: str):
        return load_moco_checkpoint(self.model.module, checkpoint_path, device=self.device)

    # ---- epochs (finetune.py:95-146, :326-376) -----------------------------------------------------------------------
    def _epoch(self, name: str, loader, n_crop: int, train: bool):
        """EpochContext.forward with its consumer folded in: one pass over `loader`.  Per iteration: model, then the fused
        criterion (crop mean, loss, gradient, accuracy over the valid samples, meters), then the optimizer when training.  The
        host reads the meters at the log interval and at the end, nowhere else.  Returns (Meters, last read)."""
        loader.set_epoch(self.current_epoch)
        meters = Meters(self.device)
        logger.info("%s epoch begin.", name)
        begin_time = time.perf_counter()
        num_iters = len(loader)
        remaining_valid_samples = loader.num_valid_samples()
        for i, ((clip,), target, *others) in enumerate(loader):
            output = self.model(reshape_clip(clip, n_crop))
            # Distributed sampler will add some repeated samples. cut them off.
            batch_size = min(target.size(0), remaining_valid_samples)
            remaining_valid_samples -= batch_size
            if batch_size == 0:
                continue
            if i > 0 and i % self.log_interval == 0:
                # numbers from the last iteration, just before this one's update (finetune.py:124-130); the one host sync
                logger.info(f"{name} [{self.current_epoch}/{self.num_epochs}][{i - 1}/{num_iters}]\t" + "\t".join(meters.pieces()))
            loss = self.criterion(output, target, n_crop=n_crop, valid=batch_size, meters=meters)
            if train:
                fp = self.fingerprints
                due = fp is not None and fp.due(self.current_epoch * num_iters + i)
                self.optimizer.zero_grad()
                loss.backward()
                if due:
                    fp.after_backward(self.model)      # (halt_on_nonfinite raises here: the parameters stay as they were)
                self.optimizer.step()
                if due:
                    fp.after_step(self.current_epoch, i, self.model)
        stats = meters.read()
        logger.info("%s epoch finished. Time: %.2f sec.\t%s\t%s\t%s", name, time.perf_counter() - begin_time, *meters.pieces(stats))
        return meters, stats

    def train_epoch(self) -> float:
        self.model.train()
        _, stats = self._epoch("Train", self.train_loader, 1, True)
        self.train_stats = stats
        return stats["acc1"]["avg"]

    def validate_epoch(self) -> float:
        self.model.eval()
        with torch.no_grad():
            meters, stats = self._epoch("Validate", self.validate_loader, self.n_crop, False)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            meters.sync_distributed()
            stats = meters.read()
        self.validate_stats = stats
        logger.info("Validation finished.\n\tLoss = %f\n\tAcc@1 = %.2f%% (%d/%d)\n\tAcc@5 = %.2f%% (%d/%d)",
                    stats["loss"]["avg"],
                    stats["acc1"]["avg"], stats["acc1"]["sum"] / 100, stats["acc1"]["count"],
                    stats["acc5"]["avg"], stats["acc5"]["sum"] / 100, stats["acc5"]["count"])
        return stats["acc1"]["avg"]

    def _write_scalars(self, lr: float):
        rec = {"epoch": self.current_epoch, "train/lr": lr}
        for prefix, stats in (("train", self.train_stats), ("val", self.validate_stats)):
            rec.update({f"{prefix}/{k}": stats[k]["avg"] for k in Meters.KEYS})
        append_scalars(self.scalars_path, rec)

    def run(self):
        num_epochs = 1 if getattr(self.args, "debug", False) else self.num_epochs
        self.model.train()
        while self.current_epoch < num_epochs:
            last_lr = getattr(self.scheduler, "_last_lr", None) or [g["lr"] for g in self.optimizer.param_groups]
            logger.info("Current LR:{}".format(last_lr))
            lr = float(self.optimizer.param_groups[0]["lr"])
            self.train_epoch()
            acc1 = self.validate_epoch()
            self._write_scalars(lr)
            if self.schedule_type == "plateau":
                self.scheduler.step(self.train_stats["loss"]["val"])
            else:
                self.scheduler.step()
            self.current_epoch += 1
            if self.local_rank == 0:
                is_best = acc1 > self.best_acc1
                self.best_acc1 = max(acc1, self.best_acc1)
                self.checkpoint_manager.save({
                    "epoch": self.current_epoch,
                    "arch": self.arch,
                    "model": self.model.module.state_dict(),
                    "best_acc1": self.best_acc1,
                    "optimizer": self.optimizer.state_dict(),
                    "scheduler": self.scheduler.state_dict(),
                }, is_best, self.current_epoch)


# ---- command line (finetune.py:426-502) ------------------------------------------------------------------------------------
def main_worker(local_rank: int, args, dist_url: str):
    setup_logging(args, local_rank)
    seed_everything(args.seed)
    torch.cuda.set_device(local_rank)
    group = init_process_group(args, local_rank, dist_url)
    cfg = load_config(args.config, args.ext_config)
    save_run(args, cfg, local_rank)
    if not args.validate:
        engine = Engine(args, cfg, local_rank=local_rank)
        if args.load_checkpoint is not None:
            engine.load_checkpoint(args.load_checkpoint)
        elif args.moco_checkpoint is not None:
            engine.load_moco_checkpoint(args.moco_checkpoint)
        engine.run()
        validate_checkpoint = Path(args.experiment_dir) / "model_best.pth.tar"
        del engine
    else:
        validate_checkpoint = args.load_checkpoint
        if not validate_checkpoint:
            raise ValueError('With "--validate" specified, you should also specify "--load-checkpoint"')
    logger.info("Doing final validate.")
    engine = Engine(args, cfg, local_rank=local_rank, final_validate=True)
    engine.load_checkpoint(validate_checkpoint)
    acc1 = engine.validate_epoch()
    finish_process_group(group)
    return acc1


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="RSPNet action-recognition fine-tuning on MI355X (flag names follow the reference's arguments.py)")
    add_driver_arguments(ap, "rspnet_amd/config/finetune/c3d.json", world_size=1)
    ap.add_argument("--moco-checkpoint", default=None, help="a pretext checkpoint: encoder_q.* feeds the backbone")
    ap.add_argument("--validate", action="store_true", help="only the final multi-crop validation of --load-checkpoint")
    ap.add_argument("--val-samples", type=int, default=100, help="synthetic validation set size")
    return parse_driver_args(ap, argv)


def main(argv=None):
    return launch(main_worker, parse_args(argv))


if __name__ == "__main__":
    main()
