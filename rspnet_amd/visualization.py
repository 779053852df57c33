"""Similarity-map pictures of a pre-trained pretext model — the reference's visualization.py minus its video
decoding and cv2.

Per batch: ``MoCoDiffLossTwoFc.cam_visualize(clip_q, clip_k, align_keys=True)`` in eval mode (rsp_cam_maps), ONE rsp_cam_overlay
launch for all 4*B panels (mean over T', min-max normalisation, bilinear resize, colour map, blend with a frame of the clip),
one device-to-host copy, then PIL writes ``iter-{i}-RSP-{rank}.png`` (the Ms_?A maps, named as visualization.py:110 names them) and
``iter-{i}-AVID-{rank}.png`` (the Ms_?M maps): query panel left, key panel right, sample 0 (``--all-samples``: every sample, with
a ``-b{b}`` suffix).

Deliberately different from visualization.py: the colour map is the analytic jet on the continuous value after
the resize (not cv2's 256-entry table applied before it), so the pictures are not pixel-identical; ``mask_clip``'s
"de-normalisation" (multiply by the mean, add the std) is not copied — the clips are un-normalised [0, 1] already, as the
reference's visualisation chain (ToTensor + Resize only) makes them; the frame drawn is the middle frame of the clip (``--frame``),
not half the channel count (``clip_q.shape[1] // 2`` = 1); key maps are paired with their own clips (align_keys).

    python -m rspnet_amd.visualization -c rspnet_amd/config/pretrain/c3d.json -e /tmp/vis --steps 2 [--load-model CKPT]
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import Iterable, Optional

import numpy as np
import torch

from . import ops as _ops
from .framework.driver import load_config, load_states, seed_everything
from .moco import ModelFactory
from .utils.moco import replace_moco_k_in_config

logger = logging.getLogger(__name__)
MARGIN, GAP, CAPTION = 10, 10, 30        # visualization.py:79-81: a (size + 40) x (2 * size + 30) white canvas
PREFIXES = ("RSP", "AVID")               # maps 0 / 2 (Ms_qA, Ms_kA) and 1 / 3 (Ms_qM, Ms_kM), as visualization.py:110-111 names them


def visualization_loader(batch_size: int, T: int, size: int, steps: int, device, seed: int = 0):
    """The synthetic uint8 video source of pretrain.py behind the reference's visualisation chain
    (datasets/classification/__init__.py:183-188: ToTensor + Resize — no grayscale, jitter or flip, mean 0, std 1): un-normalised
    [0, 1] clips."""
    from . import pretrain                       # the pretext driver owns the synthetic video source
    from .augment import FusedGPUCollateFn
    loader = pretrain.SyntheticVideoClips(batch_size, T, size, steps, device, seed=seed, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    loader.collate = FusedGPUCollateFn(size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), p_gray=0.0, brightness=0, contrast=0, saturation=0,
                                       hue=0, p_flip=0.0, target_transform=False, device=device)
    return loader


class Engine:
    """visualization.py:22-115.  ``loader`` yields ``(clip_q, clip_k)`` or the reference's ``((clip_q, clip_k), *rest)``: fp32
    (B, 3, T, size, size) clips in [0, 1]."""

    def __init__(self, args, cfg: dict, local_rank: int = 0, loader: Optional[Iterable] = None, device=None):
        self.args, self.cfg, self.local_rank = args, cfg, local_rank
        self.device = torch.device(device) if device is not None else torch.device("cuda", local_rank)
        self.model = ModelFactory(cfg).build_moco_diffloss(device=self.device)
        self.arch = cfg["arch"]
        if loader is None:
            T, size = int(cfg["temporal_transforms"]["size"]), int(cfg["spatial_transforms"]["size"])
            loader = visualization_loader(int(cfg["batch_size"]), T, size, args.steps, self.device, seed=(args.seed or 0) + local_rank)
        self.loader = loader

    def load_model(self, checkpoint_path: str):
        """visualization.py:41-50: the architecture check, then a strict load_state_dict."""
        states = load_states(checkpoint_path, self.device, self.arch)
        msg = self.model.module.load_state_dict(states["model"])
        logger.info("Missing keys: %s, Unexpected keys: %s", msg.missing_keys, msg.unexpected_keys)
        return msg

    @torch.no_grad()
    def panels(self, clip_q, clip_k) -> np.ndarray:
        """(4, B, size, size, 3) uint8 on the host, order qA, qM, kA, kM: the maps of one batch over frame `--frame` of its clips."""
        clip_q = clip_q.to(self.device, torch.float32).contiguous()
        clip_k = clip_k.to(self.device, torch.float32).contiguous()
        maps = torch.stack(self.model.module.cam_visualize(clip_q, clip_k, align_keys=True))       # (4, B, T', H', W')
        B, T = clip_q.shape[0], clip_q.shape[2]
        t = T // 2 if self.args.frame is None else int(self.args.frame)
        if not 0 <= t < T:
            raise ValueError(f"--frame {t} is outside the clip's {T} frames")
        # panels of the query clips (qA, qM) first, then of the key clips (kA, kM): one launch, one copy
        out = _ops.backend().cam_overlay(maps.reshape((4 * B,) + tuple(maps.shape[2:])), clip_q, clip_k, t)
        return out.cpu().numpy().reshape(4, B, *out.shape[1:])

    def save_fig(self, left: np.ndarray, right: np.ndarray, iteration: int, prefix: str, suffix: str = "") -> str:
        """visualization.py:76-84 with PIL: white canvas, query panel left, key panel right, captions under them when PIL's
        default font can be had (never a font file)."""
        from PIL import Image, ImageDraw
        h, w = left.shape[:2]
        canvas = np.full((h + MARGIN + CAPTION, 2 * w + 2 * MARGIN + GAP, 3), 255, dtype=np.uint8)
        canvas[MARGIN:MARGIN + h, MARGIN:MARGIN + w] = left
        canvas[MARGIN:MARGIN + h, MARGIN + GAP + w:MARGIN + GAP + 2 * w] = right
        img = Image.fromarray(canvas, "RGB")
        try:
            draw = ImageDraw.Draw(img)
            draw.text((MARGIN + w // 4, MARGIN + h + 5), f"query for {prefix}", fill=(0, 0, 0))
            draw.text((MARGIN + GAP + w + w // 4, MARGIN + h + 5), f"key for {prefix}", fill=(0, 0, 0))
        except (OSError, ImportError):          # no usable default font: the captions are optional
            pass
        path = os.path.join(self.args.experiment_dir, f"iter-{iteration}-{prefix}{suffix}-{self.local_rank}.png")
        img.save(path)
        return path

    def visual_epoch(self):
        """visualization.py:86-111.  Returns the paths written."""
        written = []
        for i, batch in enumerate(self.loader):
            if self.args.steps is not None and i >= self.args.steps:
                break
            clip_q, clip_k = batch[0] if isinstance(batch[0], (tuple, list)) else batch[:2]
            p = self.panels(clip_q, clip_k)
            for b in (range(p.shape[1]) if self.args.all_samples else (0,)):
                suffix = f"-b{b}" if self.args.all_samples else ""
                for head, prefix in enumerate(PREFIXES):
                    written.append(self.save_fig(p[head, b], p[2 + head, b], i, prefix, suffix))
        return written

    def run(self):
        self.model.eval()
        return self.visual_epoch()


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="similarity-map pictures of a pretext model (flag names follow the reference's arguments.py)")
    ap.add_argument("-c", "--config", required=True, help="resolved pretext config JSON (e.g. rspnet_amd/config/pretrain/c3d.json)")
    ap.add_argument("-x", "--ext-config", action="append", help="JSON object merged over the config (may repeat)")
    ap.add_argument("-e", "--experiment-dir", required=True, help="where the PNG files go")
    ap.add_argument("--load-model", default=None, help="a pretext checkpoint (its 'model' entry is loaded strictly)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10, help="batches to draw (synthetic loader length)")
    ap.add_argument("--frame", type=int, default=None, help="frame of the clips under the maps (default: the middle one)")
    ap.add_argument("--all-samples", action="store_true", help="a picture per sample (suffix -b{b}) instead of sample 0 only")
    return ap.parse_args(argv)


def main(argv=None, loader: Optional[Iterable] = None, device=None):
    """Single process, rank 0.  ``loader`` / ``device``: for callers with their own clips (and the host-logic tests)."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    seed_everything(args.seed)                     # utils/reproduction.py initialize_seed (visualization.py:121-122)
    cfg = load_config(args.config, args.ext_config)
    replace_moco_k_in_config(cfg)
    os.makedirs(args.experiment_dir, exist_ok=True)
    if device is None:
        torch.cuda.set_device(0)
    engine = Engine(args, cfg, 0, loader=loader, device=device)
    if args.load_model is not None:
        engine.load_model(args.load_model)
    written = engine.run()
    logger.info("wrote %d pictures to %s", len(written), args.experiment_dir)
    return written


if __name__ == "__main__":
    main()
