"""Nearest-neighbour video retrieval — the reference's retrieval.py minus its data pipeline.

Extraction (Engine): eval mode, the bare backbone's ``get_feature`` (models.feature, HIP kernels), spatial mean
(rsp_spatial_mean_fwd), mean over the crops of a sample; features stay on the device until ``save_features`` writes the
reference's files (``{train,test}_fold{F}_{feats,labels}.npy``: float64 features, as the reference's ``.tolist()`` round trip
makes them, int64 labels).  Any loader that yields ``((clip,), target)`` works; clip decoding (decord) is not rebuilt.

Search (topk_retrieval): the reference computes the full ``cosine_distances(X_test, X_train)`` matrix and argsorts it on the
host; here the k nearest gallery rows come from the fused HIP search (rsp_cosine_topk: the Nq x Ng matrix is never stored)
and the hit counts from rsp_topk_hits, so only the count vector returns to the host.  Ties between equal distances go to the
lower gallery index (numpy's argsort leaves their order undefined).

Deliberate divergence: the reference's ``.squeeze()`` turns a batch of one into a 1-D vector (its config notes "batch_size 1
cause problems"); here the pooled features are always (B, D).

    python -m rspnet_amd.retrieval --features DIR --fold F
"""
from __future__ import annotations

import argparse
import json
import logging
import os
from typing import Dict, Iterable, Sequence

import numpy as np
import torch
from torch import Tensor, nn

from . import finetune as _ft
from . import ops as _ops
from .models.feature import feature_ndhwc

logger = logging.getLogger(__name__)
KS = (1, 5, 10, 20, 50)
PREFIX = "encoder_q.encoder."
BLACKLIST = ("fc", "linear", "head", "new_fc")
_MISSING_OK = ({"fc.weight", "fc.bias"}, {"linear.weight", "linear.bias"}, {"head.projection.weight", "head.projection.bias"},
               {"new_fc.weight", "new_fc.bias"})


def feature_paths(feature_dir: str, fold: int) -> Dict[str, str]:
    return {f"{split}_{kind}": os.path.join(feature_dir, f"{split}_fold{fold}_{kind}.npy")
            for split in ("train", "test") for kind in ("feats", "labels")}


class Engine:
    """retrieval.py:35-146.  ``model`` is what models.ModelFactory.build returns (``model.module`` is the bare backbone)."""

    def __init__(self, model: nn.Module, n_crop: int = 10, fold: int = 1, device=None):
        self.model = model
        self.n_crop = int(n_crop)
        self.fold = int(fold)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.feats = {"train": [], "test": []}
        self.labels = {"train": [], "test": []}

    def reshape_clip(self, clip: Tensor) -> Tensor:
        """(B, C, n_crop*T, H, W) -> (B*n_crop, C, T, H, W), crops of one sample adjacent (retrieval.py:65-73)."""
        return _ft.reshape_clip(clip, self.n_crop)

    def average_clips(self, feats: Tensor) -> Tensor:
        """(B*n_crop, D) -> (B, D), mean over the crops of a sample (retrieval.py:75-82)."""
        return _ft.average_logits(feats, self.n_crop)

    def load_moco_checkpoint(self, checkpoint_path: str):
        """retrieval.py:84-101: the pretext checkpoint's ``encoder_q.encoder.*`` minus the classifier-like names, loaded
        non-strictly into the bare backbone; exactly one classifier's weight and bias may be missing."""
        cp = torch.load(checkpoint_path, map_location=self.device, weights_only=False)
        logger.info("Loading MoCo checkpoint from %s (epoch %d)", checkpoint_path, cp["epoch"])
        state = {k[len(PREFIX):]: v for k, v in cp["model"].items()
                 if k.startswith(PREFIX) and not any(k.startswith(PREFIX + b) for b in BLACKLIST)}
        msg = self.model.module.load_state_dict(state, strict=False)
        assert set(msg.missing_keys) in _MISSING_OK, msg
        return msg

    @torch.no_grad()
    def features(self, clip: Tensor) -> Tensor:
        """One batch: (B, C, n_crop*T, H, W) -> (B, D) on the device (always 2-D, also for B = 1)."""
        backbone = self.model.module
        feat = feature_ndhwc(backbone, self.reshape_clip(clip.to(self.device, torch.float32)))
        return self.average_clips(_ops.backend().spatial_mean_fwd(feat))

    @torch.no_grad()
    def extract_features(self, loader: Iterable, split: str):
        """retrieval.py:103-131 for ``split`` in {"train", "test"}: eval mode, features of every batch kept on the device."""
        if split not in self.feats:
            raise ValueError(f"split must be 'train' or 'test', not {split!r}")
        self.model.eval()
        for (clip,), target in loader:
            self.feats[split].append(self.features(clip))
            self.labels[split].append(torch.as_tensor(target).to(self.device, torch.int64).reshape(-1))

    def split_tensors(self, split: str):
        return torch.cat(self.feats[split]), torch.cat(self.labels[split])

    def save_features(self, save_dir: str):
        """retrieval.py:134-145: the reference's file names and dtypes (float64 features, int64 labels)."""
        os.makedirs(save_dir, exist_ok=True)
        paths = feature_paths(save_dir, self.fold)
        logger.info("Saving features for train and test splits in %s...", save_dir)
        for split in ("train", "test"):
            f, y = self.split_tensors(split)
            np.save(paths[f"{split}_feats"], f.cpu().numpy().astype(np.float64))
            np.save(paths[f"{split}_labels"], y.cpu().numpy().astype(np.int64))
        logger.info("Saving features done.")

    def run(self, feat_dir: str, train_loader: Iterable, test_loader: Iterable):
        """retrieval.py:147-151 with the loaders passed in: extract both splits, save them."""
        self.extract_features(train_loader, "train")
        self.extract_features(test_loader, "test")
        self.save_features(feat_dir)


def search(X_test, y_test, X_train, y_train, ks: Sequence[int] = KS, device=None) -> Dict[int, int]:
    """Top-k hit counts of the test rows against the train rows (retrieval.py:161-176) on the HIP search kernels."""
    be = _ops.backend()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    q = torch.as_tensor(np.asarray(X_test), dtype=torch.float32).to(dev).contiguous()
    g = torch.as_tensor(np.asarray(X_train), dtype=torch.float32).to(dev).contiguous()
    yq = torch.as_tensor(np.asarray(y_test), dtype=torch.int64).to(dev).contiguous()
    yg = torch.as_tensor(np.asarray(y_train), dtype=torch.int64).to(dev).contiguous()
    idx, _ = be.cosine_topk(q, g, max(ks))
    counts = be.topk_hits(idx, yq, yg, list(ks)).cpu().tolist()
    return {int(k): int(c) for k, c in zip(ks, counts)}


def topk_retrieval(feature_dir: str, fold: int, ks: Sequence[int] = KS, device=None) -> Dict[int, int]:
    """retrieval.py:153-183: load the saved features, search on the GPU, log the reference's lines and write
    ``topk_correct_fold{F}.json`` byte for byte as its ``json.dump`` does.  Returns {k: correct}."""
    logger.info("Loading local .npy files...")
    X_train, y_train, X_test, y_test = load_features(feature_dir, fold)
    topk_correct = search(X_test, y_test, X_train, y_train, ks, device)
    total = len(X_test)
    for k in ks:
        correct = topk_correct[k]
        logger.info("Top-{}, correct = {:.2f}, total = {}, acc = {:.3f}".format(k, correct, total, correct / total))
    write_topk_json(feature_dir, fold, topk_correct)
    return topk_correct


def load_features(feature_dir: str, fold: int):
    """(X_train, y_train, X_test, y_test) from the reference's files (retrieval.py:157-163)."""
    p = feature_paths(feature_dir, fold)
    return np.load(p["train_feats"]), np.load(p["train_labels"]), np.load(p["test_feats"]), np.load(p["test_labels"])


def write_topk_json(feature_dir: str, fold: int, topk_correct: Dict[int, int]) -> str:
    """``topk_correct_fold{F}.json`` as the reference's ``json.dump`` of its {k: count} dict writes it (retrieval.py:181-182)."""
    path = os.path.join(feature_dir, f"topk_correct_fold{fold}.json")
    with open(path, "w") as fp:
        json.dump({int(k): int(v) for k, v in topk_correct.items()}, fp)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description="top-k video retrieval over a directory of saved features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="comma-separated k values (each <= 64)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    topk_retrieval(args.features, args.fold, [int(k) for k in args.ks.split(",")])


if __name__ == "__main__":
    main()
