"""Pretext-training driver for rspnet_amd — the `pretrain.py` surface of the reference (config keys, CLI flag names,
checkpoint layout, LR policy) around the MI355X-native step.

Mirrors /root/reference/pretrain.py:31-336 for what touches the hot path: Engine construction (:33-110: model factory,
Loss(margin=2.0, A, M), LR scaling, SGD, CosineAnnealingLR per epoch with eta_min = lr/1000), checkpoint load with the arch
check (:112-132), the train loop (:147-218: forward, loss, zero_grad/backward/step or `--validate`, the top-k accuracies and the
eight meters as ONE HIP call per step, rsp_pretext_metrics, the log wording, per-epoch scalars to scalars.jsonl), epoch loop and
checkpoint dict (:220-260), one process per GPU started with mp.spawn and a tcp://127.0.0.1 rendezvous (:263-336).
The data pipeline (decord decode + GPU augmentation) is out of scope: the loader here is any iterable
of (clip_q, clip_k) device tensors; `SyntheticClips` stands in for it.  The config is the resolved JSON the reference
saves as run_*/config.json (rspnet_amd/config/pretrain/*.json ship the four shipped pretext configs).
"""
from __future__ import annotations

import argparse
import json
import logging
import math
import os
import time
from pathlib import Path

import torch

from . import _lib, fingerprint, ops
from .cluster import ClusterMonitor
from .framework.arguments import RUN_DIR_NAME_REGEX, add_driver_arguments, parse_driver_args, save_run_files  # noqa: F401
from .framework.driver import (append_scalars, finish_process_group, init_process_group, launch, load_config, load_states, save_run,
                               seed_everything, setup_logging, visible_gpu_count)
from .framework.meters import DeviceMeters
from .framework.utils.checkpoint import CheckpointManager
from .framework.utils.environment import scale_learning_rate
from .knn import KNNMonitor
from .linear_probe import LinearProbeMonitor
from .moco import Loss, ModelFactory
from .optim import SGD
from .repr_stats import ReprMonitor
from .tsne import TsneMonitor
from .utils.moco import replace_moco_k_in_config

logger = logging.getLogger(__name__)

# The opt-in epoch-end monitors (framework/monitor.py), in the order they run and their scalars are written.  Each is its config key
# (the class's KEY) away, e.g. -x '{KEY: {"every": 10}}'; a new one is a subclass of EpochMonitor appended here.
MONITORS = (KNNMonitor, ReprMonitor, LinearProbeMonitor, ClusterMonitor, TsneMonitor)


def accuracy(output: torch.Tensor, target: torch.Tensor, topk=(1,)):
    """Top-k hit rate x100 (framework/metrics/classification.py:6-20); stays on device (no sync)."""
    maxk = max(topk)
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    return [correct[:k].reshape(-1).float().sum(0) * (100.0 / target.size(0)) for k in topk]


def pretext_accuracy(output, ranking_logits) -> torch.Tensor:
    """(acc1_A, acc5_A, acc1_A_n, acc5_A_n, acc1_M) in percent as one (5,) tensor: what pretrain.py:169-172 takes from
    accuracy(output[0], 0, (1, 5)), accuracy(output[1], 0, (1, 5)) and accuracy(cat(ranking_logits), 0, (1,)), restated on the rank of
    the positive (column 0), rank = #{c : v[c] > v[0]}, with the tie rule of rsp_pretext_metrics: a column equal to the positive does
    not count, a NaN positive is a miss, l_pos_M == l_neg_M is a hit.  Torch ops, any device; no sync."""
    B = output[0].shape[0]
    hits = []
    for logits in output:
        pos = logits[:, :1]
        rank = (logits > pos).sum(dim=1)
        ok = (pos == pos).view(-1)
        hits += [((rank == 0) & ok).sum(), ((rank < 5) & ok).sum()]
    hits.append((ranking_logits[0].reshape(-1) >= ranking_logits[1].reshape(-1)).sum())
    return torch.stack(hits).to(torch.float32) * (100.0 / B)                      # classification.py:18-19


class PretextMeters(DeviceMeters):
    """The eight running meters of a pretext epoch (pretrain.py:97-106) over rsp_pretext_meters; rsp_pretext_metrics updates them on
    the device."""

    NAMES = ("Loss", "Loss_A", "Acc@1_A", "Acc@5_A", "Acc@1_A_n", "Acc@5_A_n", "Loss_M", "Acc@1_M")
    KEYS = ("loss", "loss_A", "acc1_A", "acc5_A", "acc1_A_n", "acc5_A_n", "loss_M", "acc1_M")
    FMTS = (":f", ":f", ":6.2f", ":6.2f", ":6.2f", ":6.2f", ":f", ":6.2f")
    STRUCT = _lib.PretextMeters


def _losses3(loss, loss_A, loss_M) -> torch.Tensor:
    """The step's (loss, loss_A, loss_M) as one (3,) tensor: the buffer rsp_loss_fwd_bwd wrote when the three are its elements (no
    launch), a stack otherwise."""
    loss = loss.detach()
    if (loss.dim() == 0 and loss.dtype == torch.float32 and loss_A.data_ptr() == loss.data_ptr() + 4
            and loss_M.data_ptr() == loss.data_ptr() + 8):
        return torch.as_strided(loss, (3,), (1,), loss.storage_offset())
    return torch.stack([loss, loss_A.detach(), loss_M.detach()]).to(torch.float32)


class SyntheticClips:
    """Stand-in data loader: `steps` batches of N(0,1) clip pairs (B,3,T,H,W), generated once on the device."""

    def __init__(self, batch_size, T, size, steps, device, seed=1234):
        g = torch.Generator(device=device).manual_seed(seed)
        self.q = torch.randn(batch_size, 3, T, size, size, device=device, generator=g)
        self.k = torch.randn(batch_size, 3, T, size, size, device=device, generator=g)
        self.steps = steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.q, self.k


class SyntheticVideoClips:
    """Decode-free stand-in for the reference's video pipeline that still exercises its GPU half: every step yields B samples
    of two uint8 (T, h, w, 3) crops -- a fixed pool of synthetic "videos", a RawVideoRandomCrop window (scale 0.4..1, aspect
    3/4..4/3; transforms_spatial.py:43-80) drawn per clip on the CPU as the reference does -- and hands them to
    rspnet_amd.augment.FusedGPUCollateFn (ToTensor, Resize, grayscale, colour jitter, flip, normalise in one HIP launch group),
    i.e. the loader returns (clip_q, clip_k) device tensors exactly like DataLoader(collate_fn=SequentialGPUCollateFn(...))."""

    def __init__(self, batch_size, T, size, steps, device, seed=1234, src_hw=(128, 171), mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), aug_plus=False, pool=8):
        import random as _random
        from .augment import FusedGPUCollateFn
        g = torch.Generator().manual_seed(seed)
        self.videos = [torch.randint(0, 256, (T, src_hw[0], src_hw[1], 3), dtype=torch.uint8, generator=g) for _ in range(pool)]
        self.collate = FusedGPUCollateFn(size, mean, std, target_transform=False, device=device, aug_plus=aug_plus)
        self.batch_size, self.steps = batch_size, steps
        self.rng = _random.Random(seed)

    def _crop(self, clip):
        H, W = clip.shape[1], clip.shape[2]
        for _ in range(10):
            area = self.rng.uniform(0.4, 1.0) * H * W
            ar = math.exp(self.rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 0 < w <= W and 0 < h <= H:
                i, j = self.rng.randint(0, H - h), self.rng.randint(0, W - w)
                return clip[:, i:i + h, j:j + w, :].contiguous()
        return clip

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            batch = []
            for _b in range(self.batch_size):
                v = self.videos[self.rng.randrange(len(self.videos))]
                batch.append(([self._crop(v), self._crop(v)], 0))
            (clip_q, clip_k), _ = self.collate(batch)
            yield clip_q, clip_k


class Engine:
    def __init__(self, args, cfg: dict, local_rank: int, train_loader=None, knn_loaders=None):
        self.args, self.cfg, self.local_rank = args, cfg, local_rank
        self._stepper, self._first_epoch = None, 0
        self.device = torch.device("cuda", local_rank)
        self.model = ModelFactory(cfg).build_moco_diffloss(device=self.device)
        self.criterion = Loss(margin=2.0, A=float(cfg["loss_lambda"]["A"]), M=float(cfg["loss_lambda"]["M"]))
        self.batch_size = int(cfg["batch_size"])
        self.learning_rate = float(cfg["optimizer"]["lr"])
        if not args.no_scale_lr:
            self.learning_rate = scale_learning_rate(self.learning_rate, args.world_size, self.batch_size)
        o = cfg["optimizer"]
        # all parameters, frozen encoder_k included, exactly as pretrain.py:65-72 does: the checkpoint's 'optimizer' entry
        # (param_groups[0]['params'] indices) is then interchangeable with the reference's
        self.optimizer = SGD(self.model.parameters(), lr=self.learning_rate,
                             momentum=float(o["momentum"]), dampening=float(o["dampening"]),
                             weight_decay=float(o["weight_decay"]), nesterov=bool(o["nesterov"]))
        self.num_epochs = int(cfg["num_epochs"])          # the jsonnet value is the STRING '200' (moco-train-base.jsonnet:18)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=self.num_epochs,
                                                                    eta_min=self.learning_rate / 1000)
        self.arch = cfg["arch"]
        self.checkpoint = (CheckpointManager(args.experiment_dir, keep_interval=int(cfg["checkpoint_interval"]))
                           if local_rank == 0 else None)
        self.log_interval = int(cfg["log_interval"])
        self.current_epoch = 0
        self.best_loss = math.inf
        self.meters, self.stats = None, None
        run_dir = getattr(args, "run_dir", None)
        self.scalars_path = None if run_dir is None or local_rank != 0 else Path(run_dir) / "scalars.jsonl"
        # opt-in (config key "fingerprint", e.g. -x '{"fingerprint": {"every": 50, "halt_on_nonfinite": true}}'): None otherwise
        self.fingerprints = fingerprint.StepFingerprints.from_config(cfg, run_dir, rank=local_rank)
        T, size = int(cfg["temporal_transforms"]["size"]), int(cfg["spatial_transforms"]["size"])
        if train_loader is None and getattr(args, "loader", "tensor") == "uint8":
            train_loader = SyntheticVideoClips(self.batch_size, T, size, args.steps_per_epoch, self.device,
                                               seed=args.seed + local_rank, aug_plus=bool(cfg.get("moco", {}).get("aug_plus", False)))
        self.train_loader = train_loader or SyntheticClips(self.batch_size, T, size, args.steps_per_epoch, self.device,
                                                           seed=args.seed + local_rank)
        # MONITORS: built on every rank (None for a key the config does not carry); rank 0 runs them on loaders of its own -- the
        # stand-in labelled clips of each monitor, or knn_loaders: a (bank, query) pair yielding ((clip,), target) for the kNN monitor
        self.monitors = [m for m in (cls.from_config(cfg, self.num_epochs) for cls in MONITORS) if m is not None]
        self.monitor_loaders, self.monitor_results = {}, {}
        for m in self.monitors:
            if knn_loaders is not None and isinstance(m, KNNMonitor):
                self.monitor_loaders[m.KEY] = tuple(knn_loaders)
            elif local_rank == 0:
                self.monitor_loaders[m.KEY] = m.build_loaders(T, size, self.device, seed=args.seed)

    # ---- checkpoints (pretrain.py:112-132) ---------------------------------------------------------------------------
    def load_checkpoint(self, path):
        states = load_states(path, self.device, self.arch)
        self.model.module.load_state_dict(states["model"])
        self.optimizer.load_state_dict(states["optimizer"])
        self.scheduler.load_state_dict(states["scheduler"])
        self.current_epoch = states["epoch"]
        self.best_loss = states["best_loss"]

    def load_model(self, path):
        self.model.module.load_state_dict(load_states(path, self.device, self.arch)["model"])

    # ---- training (pretrain.py:147-260) ------------------------------------------------------------------------------
    def _update_meters(self, loss, loss_A, loss_M, output, ranking_logits):
        """The step's accuracies and the eight meter updates (pretrain.py:167-195): ONE rsp_pretext_metrics call, issued behind the
        step; torch ops on a backend without the entry point."""
        be = ops.backend()
        if hasattr(be, "pretext_metrics"):
            be.pretext_metrics(output[0].contiguous(), output[1].contiguous(), ranking_logits[0].contiguous(),
                               ranking_logits[1].contiguous(), _losses3(loss, loss_A, loss_M), self.meters.buf)
        else:
            acc = pretext_accuracy(output, ranking_logits)
            self.meters.update([loss, loss_A, acc[0], acc[1], acc[2], acc[3], loss_M, acc[4]], output[0].shape[0])

    def train_epoch(self, validate: bool = False):
        """One pass over the loader (pretrain.py:147-218).  validate (--validate, :162): forward, loss and meters only -- no
        zero_grad / backward / step and no graph capture; the model's own state (key encoder, queue, BatchNorm statistics) moves as
        a forward moves it, the parameters of encoder_q do not change."""
        if self.meters is None:
            self.meters = PretextMeters(self.device)
        self.meters.reset()
        n = 0
        num_iters = len(self.train_loader)
        t0 = time.perf_counter()
        if (not validate and self._stepper is None and self.device.type == "cuda"
                and not getattr(self.args, "no_graph", False)):
            # the five statements below run through the stepper — replayed as linear HIP graphs on three streams, with the
            # data-parallel collectives between them at more than one rank, where the host cannot issue the step fast enough; the
            # eager loop with its side streams otherwise (rspnet_amd/graph_step.py)
            from .graph_step import GraphedPretextStep
            self._stepper = GraphedPretextStep(self.model, self.criterion, self.optimizer)
        for it, (clip_q, clip_k) in enumerate(self.train_loader):
            if it == 2 and self.current_epoch == self._first_epoch:
                # modules, layer plans and descriptor caches are long-lived: park them in the permanent generation so a full
                # garbage collection cannot pause the host for tens of ms while the GPU runs dry (measured: 40-75 ms, bench.py)
                import gc
                gc.collect()
                gc.freeze()
            if self._stepper is not None and not validate:
                loss, loss_A, loss_M, output, ranking_logits = self._stepper(clip_q, clip_k)
            else:
                output, target, ranking_logits, ranking_target = self.model(clip_q, clip_k)
                loss, loss_A, loss_M = self.criterion(output, target, ranking_logits, ranking_target)
                if not validate:
                    self.optimizer.zero_grad()
                    loss.backward()
                    self.optimizer.step()
            if self.local_rank == 0 and it > 0 and it % self.log_interval == 0:
                # numbers from the last iteration, just before this one's update (pretrain.py:177-185); the only host sync
                p = self.meters.pieces()
                logger.info(f"Train [{self.current_epoch}/{self.num_epochs}][{it - 1}/{num_iters}]"
                            f"\t{p[1]}\t{p[2]}\t{p[3]}\n{p[6]}\t{p[7]}\n{p[4]}\t{p[5]}")
            # the stepper's tensors are the graphs' output buffers: consumed here, before the next step overwrites them
            self._update_meters(loss, loss_A, loss_M, output, ranking_logits)
            fp = self.fingerprints
            if fp is not None and fp.due(self.current_epoch * num_iters + it):
                # behind the step, eagerly on its stream (never captured): the gradients are still in g_flat, the state is as updated.
                # --validate: state only.  A halt leaves this epoch's checkpoint unwritten.
                if not validate:
                    fp.after_backward(self.model)
                fp.after_step(self.current_epoch, it, self.model)
            n += 1
        torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - t0
        self.stats = self.meters.read()
        out = {k: self.stats[k]["avg"] for k in ("loss", "loss_A", "loss_M", "acc1_A", "acc5_A", "acc1_A_n", "acc5_A_n", "acc1_M")}
        out["clips_per_s"] = n * self.batch_size * self.args.world_size / dt
        return out

    def _write_scalars(self, lr: float):
        """One line per epoch in RUN_DIR/scalars.jsonl (rank 0): what pretrain.py:199-218,240 hands to the summary writer."""
        rec = {"epoch": self.current_epoch, "train/lr": lr}
        rec.update({f"train/{k}": self.stats[k]["avg"] for k in ("loss", "loss_A", "acc1_A", "acc5_A", "loss_M", "acc1_M")})
        for m in self.monitors:
            if m.KEY in self.monitor_results:
                rec.update(m.scalars(self.monitor_results[m.KEY]))
        append_scalars(self.scalars_path, rec)

    def _run_monitors(self):
        """After the epoch's last step (train_epoch has waited for it) and before its scalar line, every due monitor in list order: rank 0
        runs it eagerly on the current stream (nothing here is captured) and logs its line; the other ranks wait at a barrier, one per
        due monitor.  The monitors have run on one GPU only."""
        self.monitor_results = {}
        due = [m for m in self.monitors if m.due(self.current_epoch)]
        ctx = {"epoch": self.current_epoch, "num_epochs": self.num_epochs, "run_dir": os.path.dirname(str(self.scalars_path)),
               "due": tuple(m.KEY for m in due)}
        for m in due:
            if self.local_rank == 0:
                r = self.monitor_results[m.KEY] = m.run_epoch(self.model, self.monitor_loaders[m.KEY], ctx)
                logger.info(m.log_line(r, ctx))
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                torch.distributed.barrier()

    def run(self):
        num_epochs = 1 if self.args.debug else self.num_epochs
        self._first_epoch = self.current_epoch
        self.model.train()
        stats = None
        if getattr(self.args, "validate", False):
            # --validate (pretrain.py:162): the loop body without the optimisation; one epoch, nothing is saved
            stats = self.train_epoch(validate=True)
            if self.local_rank == 0:
                logger.info("validate epoch %d done: %s", self.current_epoch, json.dumps(stats))
            return stats
        while self.current_epoch < num_epochs:
            lr = float(self.optimizer.param_groups[0]["lr"])
            stats = self.train_epoch()
            self._run_monitors()
            self.scheduler.step()
            self._write_scalars(lr)
            self.current_epoch += 1
            self.model.sync_buffers()
            if self.local_rank == 0:
                is_best = stats["loss"] < self.best_loss
                self.best_loss = min(self.best_loss, stats["loss"])
                self.checkpoint.save({"epoch": self.current_epoch, "arch": self.arch,
                                      "model": self.model.module.state_dict(), "best_loss": self.best_loss,
                                      "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict()},
                                     is_best, self.current_epoch)
                logger.info("epoch %d done: %s", self.current_epoch, json.dumps(stats))
        return stats


def main_worker(local_rank: int, args, dist_url: str):
    setup_logging(args, local_rank)
    seed_everything(args.seed + local_rank)                         # utils/reproduction.py initialize_seed (pretrain.py:266-267)
    torch.cuda.set_device(local_rank)
    forced = args.world_size <= 1 and bool(os.environ.get("RSP_FORCE_COLLECTIVES"))      # one rank, RCCL path on (see MoCoDiffLossTwoFc)
    group = init_process_group(args, local_rank, dist_url, forced)
    cfg = load_config(args.config, args.ext_config)
    replace_moco_k_in_config(cfg)
    save_run(args, cfg, local_rank)
    engine = Engine(args, cfg, local_rank)
    if args.load_model is not None:
        engine.load_model(args.load_model)
    if args.load_checkpoint is not None:
        engine.load_checkpoint(args.load_checkpoint)
    stats = engine.run()
    finish_process_group(group)
    return stats


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="RSPNet pretext training on MI355X (flag names follow the reference's arguments.py)")
    add_driver_arguments(ap, "rspnet_amd/config/pretrain/c3d.json", world_size=None)
    ap.add_argument("--load-model", default=None)
    ap.add_argument("--no-scale-lr", action="store_true")
    ap.add_argument("--validate", action="store_true",
                    help="one epoch of forward, loss and meters without optimisation (pretrain.py:162)")
    ap.add_argument("--no-graph", action="store_true", help="never replay the step as captured HIP graphs (default: only when the host is the limiter)")
    ap.add_argument("--loader", choices=("tensor", "uint8"), default="tensor",
                    help="tensor: fixed N(0,1) device clips; uint8: synthetic uint8 videos -> CPU random crop -> fused GPU augmentation")
    args = parse_driver_args(ap, argv)
    if args.world_size is None:
        args.world_size = visible_gpu_count()
    return args


def main(argv=None):
    # Unlike the reference (which needs >= 2 ranks for shuffle-BN unless --debug), one GPU is a supported configuration.
    return launch(main_worker, parse_args(argv))


if __name__ == "__main__":
    main()
