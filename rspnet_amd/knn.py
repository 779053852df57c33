"""Weighted kNN classifier of instance discrimination: a training-free read of representation quality for a pretext run.  The
project's own (the reference has no such monitor); the rule is the one MoCo-style code uses.

Features of a labelled bank and of a labelled query set come from the backbone in eval mode (``extract``); every query's k cosine
neighbours in the bank vote for their class with weight ``exp(s / T)``; top-1 / top-5 accuracy of the queries' own labels is the
result.  On the HIP backend the search, the vote, the rank of the target and the hit counts are ONE call (rsp_knn_classify,
csrc/cos_search.hip, csrc/knn.hip): the Nq x Ng similarity matrix is never stored.

The rule (include/rspnet_hip.h states it for the kernel; ``knn_reference`` restates it in numpy fp64):

    s          (q.g) * (1/|q|) * (1/|g|); a zero-norm row has inverse norm 0
    neighbours the k rows of largest s; an exact tie goes to the lower gallery index; with Ng < k only Ng exist and vote
    w_j        exp((s_j - 1) / T): every class of a query is scaled by the same exp(-1/T), the ranking is that of exp(s_j / T)
    votes[c]   sum of w_j over the neighbours with label c (fp32, in neighbour-rank order on the device); a gallery label outside
               [0, num_classes) casts no vote
    pred       the class of the largest vote, a tie to the lower class index
    rank       #{c : v[c] > v[t]} + #{c < t : v[c] == v[t]} for the query's label t (the tie rule of rsp_xent_metrics); num_classes
               -- a miss -- for a label outside [0, num_classes)
    hits       queries i < valid with rank < 1, and with rank < 5

Limits of the kernel, enforced here as well: 1 <= k <= 256, 1 <= num_classes <= 1024, T finite and >= 0.01.

``KNNMonitor`` is the pretext driver's opt-in hook (config key ``knn_monitor``); ``python -m rspnet_amd.knn --features DIR --fold F``
classifies the test features ``rspnet_amd.retrieval`` saved against its train features.  The monitor has run on one GPU only.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import logging
import math
import os
import time
from typing import Iterable, Optional

import numpy as np
import torch
from torch import Tensor, nn

from . import finetune as _ft
from . import ops as _ops
from .framework.monitor import EpochMonitor

logger = logging.getLogger(__name__)
MAX_K, MAX_CLASSES, MIN_T = 256, 1024, 0.01


def check_limits(k, t, num_classes):
    """ValueError for values rsp_knn_classify would reject."""
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"knn: k must be in [1, {MAX_K}], got {k}")
    if not (math.isfinite(float(t)) and float(t) >= MIN_T):
        raise ValueError(f"knn: T must be finite and >= {MIN_T}, got {t}")
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"knn: num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")


# ---- the definition in numpy fp64 ----------------------------------------------------------------------------------------
def knn_reference(q, y_q, g, y_g, k: int, T: float, num_classes: int):
    """The rule of the module docstring in numpy fp64.  Returns (rank (Nq,) int64, votes (Nq, num_classes) fp64, topk_idx (Nq, k)
    int64 -- -1 past Ng --, topk_sim (Nq, k) fp64 -- -inf past Ng --, next_sim (Nq,): the similarity of the (k+1)-th neighbour,
    -inf when there is none)."""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    y_q, y_g = np.asarray(y_q, dtype=np.int64).reshape(-1), np.asarray(y_g, dtype=np.int64).reshape(-1)
    Nq, Ng, C = q.shape[0], g.shape[0], int(num_classes)
    nq, ng = np.linalg.norm(q, axis=1, keepdims=True), np.linalg.norm(g, axis=1, keepdims=True)
    sim = (q * np.where(nq > 0, 1.0 / np.where(nq > 0, nq, 1.0), 0.0)) @ (g * np.where(ng > 0, 1.0 / np.where(ng > 0, ng, 1.0), 0.0)).T
    order = np.lexsort((np.broadcast_to(np.arange(Ng), sim.shape), -sim), axis=1)      # s descending, then index ascending
    ssim = np.take_along_axis(sim, order, axis=1)
    kk = min(int(k), Ng)
    topk_idx = np.full((Nq, k), -1, dtype=np.int64)
    topk_sim = np.full((Nq, k), -np.inf)
    topk_idx[:, :kk], topk_sim[:, :kk] = order[:, :kk], ssim[:, :kk]
    next_sim = ssim[:, kk] if Ng > kk else np.full(Nq, -np.inf)
    w = np.exp((ssim[:, :kk] - 1.0) / float(T))
    lab = y_g[order[:, :kk]]
    ok = (lab >= 0) & (lab < C)
    votes = np.zeros((Nq, C))
    rows = np.broadcast_to(np.arange(Nq)[:, None], lab.shape)
    np.add.at(votes, (rows[ok], lab[ok]), w[ok])
    good = (y_q >= 0) & (y_q < C)
    t = np.where(good, y_q, 0)
    vt = votes[np.arange(Nq), t][:, None]
    cls = np.arange(C)[None, :]
    rank = ((votes > vt) | ((votes == vt) & (cls < t[:, None]))).sum(axis=1)
    return np.where(good, rank, C).astype(np.int64), votes, topk_idx, topk_sim, next_sim


# ---- the classifier ------------------------------------------------------------------------------------------------------
def _knn_torch(q: Tensor, y_q: Tensor, g: Tensor, y_g: Tensor, k: int, T: float, C: int):
    """The same rule from torch ops on whatever device the tensors are on (this one stores the Nq x Ng matrix): (pred, rank, votes)."""
    def inv(x):
        n = x.norm(dim=1, keepdim=True)
        return torch.where(n > 0, 1.0 / n, torch.zeros_like(n))
    sim = (q @ g.t()) * inv(q) * inv(g).t()
    sim = torch.where(sim == sim, sim, torch.full_like(sim, -math.inf))            # a NaN similarity never enters a list
    vals, idx = sim.topk(min(k, g.shape[0]), dim=1)
    idx, o1 = idx.sort(dim=1, stable=True)                                         # re-sort by (-s, index): torch.topk leaves ties open
    vals, o2 = vals.gather(1, o1).sort(dim=1, descending=True, stable=True)
    idx = idx.gather(1, o2)
    lab = y_g[idx]
    ok = (lab >= 0) & (lab < C) & (vals > -math.inf)
    w = torch.exp((vals - 1.0) * np.float32(1.0 / np.float32(T))) * ok
    votes = torch.zeros((q.shape[0], C), dtype=torch.float32, device=q.device).scatter_add_(1, lab.clamp(0, C - 1), w)
    good = (y_q >= 0) & (y_q < C)
    rank = torch.where(good, _ft.rank_of_target(votes, y_q.clamp(0, C - 1)), torch.full_like(y_q, C))
    return votes.argmax(dim=1), rank, votes       # (argmax: the first maximum -- the lower class -- on the backends this runs on)


def knn_classify(q: Tensor, y_q: Tensor, g: Tensor, y_g: Tensor, k: int = 200, T: float = 0.07, num_classes: Optional[int] = None,
                 valid: Optional[int] = None) -> dict:
    """Weighted kNN accuracy of the query rows q (Nq, D) with labels y_q against the bank g (Ng, D) with labels y_g.  Returns
    {"acc1", "acc5" (percent over the first ``valid`` queries), "hits" (hits1, hits5), "n", "pred", "rank"}.  One rsp_knn_classify
    call when the active op backend has ``knn_classify``; the same rule from torch ops otherwise."""
    if num_classes is None:
        num_classes = int(max(int(y_q.max()), int(y_g.max()))) + 1
    check_limits(k, T, num_classes)
    Nq = q.shape[0]
    n = Nq if valid is None else int(valid)
    if not 0 <= n <= Nq:
        raise ValueError(f"knn: valid must be in [0, {Nq}], got {valid}")
    q, g = q.to(torch.float32), g.to(torch.float32)
    y_q, y_g = y_q.to(torch.int64).reshape(-1).contiguous(), y_g.to(torch.int64).reshape(-1).contiguous()
    be = _ops.backend()
    if hasattr(be, "knn_classify"):
        res = be.knn_classify(q, g, y_g, int(k), float(T), int(num_classes), y_q=y_q, valid=n)
        pred, rank = res.pred, res.rank
        h1, h5 = (int(v) for v in res.hits.cpu().tolist())
    else:
        pred, rank, _ = _knn_torch(q, y_q, g, y_g, int(k), float(T), int(num_classes))
        h1, h5 = int((rank[:n] < 1).sum()), int((rank[:n] < 5).sum())
    return {"acc1": 100.0 * h1 / n if n else 0.0, "acc5": 100.0 * h5 / n if n else 0.0, "hits": (h1, h5), "n": n, "pred": pred,
            "rank": rank}


# ---- features ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def extract(encoder: nn.Module, loader: Iterable, device, n_crop: int = 1):
    """(features (N, D), labels (N,)) of every sample of ``loader`` (batches ``((clip,), target)``), both on the device: the
    MultiTaskWrapper's backbone in eval mode on the HIP kernels (``features_ndhwc``: neither the heads nor ``encoder.feat`` are
    touched), spatial mean, mean over the ``n_crop`` crops of a sample."""
    be = _ops.backend()
    feats, labels = [], []
    for (clip,), target in loader:
        x = _ft.reshape_clip(clip.to(device, torch.float32), n_crop)
        fmap = encoder.features_ndhwc(encoder._to_ndhwc(x), training=False)
        feats.append(_ft.average_logits(be.spatial_mean_fwd(fmap), n_crop))
        labels.append(torch.as_tensor(target).to(device, torch.int64).reshape(-1))
    return torch.cat(feats), torch.cat(labels)


def synthetic_loaders(bank_samples: int, query_samples: int, batch_size: int, num_classes: int, n_crop: int, T: int, size: int, device,
                      seed: int = 0):
    """The monitors' stand-in data: two ``SyntheticLabelledClips``, bank = split 'train' (order fixed by its epoch 0), query = split
    'val'."""
    bank = _ft.SyntheticLabelledClips("train", bank_samples, min(batch_size, bank_samples), num_classes, T, size, device, n_crop=n_crop,
                                      seed=seed)
    query = _ft.SyntheticLabelledClips("val", query_samples, batch_size, num_classes, T, size, device, n_crop=n_crop, seed=seed)
    return bank, query


@contextlib.contextmanager
def frozen_encoder(model: nn.Module, encoder: str):
    """Encoder 'q' or 'k' of the pretext model (or its wrapper with ``.module``) with the whole model in eval mode; every module's
    ``training`` flag is put back on the way out.  What every monitor that extracts features goes through."""
    net = getattr(model, "module", model)
    flags = [(m, m.training) for m in net.modules()]
    try:
        net.eval()
        if encoder == "q" and hasattr(net, "_check_q_weights"):      # a torch-side optimizer leaves the re-pack to the next forward
            if not net._q_params:
                net._q_params = list(net.encoder_q.parameters())
            net._check_q_weights()
        yield net.encoder_q if encoder == "q" else net.encoder_k
    finally:
        for m, was in flags:
            m.training = was


def extract_bank(enc: nn.Module, bank_loader: Iterable, n_crop: int = 1):
    """``extract`` of a bank through the encoder ``frozen_encoder`` yields; a bank of split 'train' has n_crop = 1 clips."""
    n_crop_bank = 1 if getattr(bank_loader, "split", None) == "train" else n_crop
    return extract(enc, bank_loader, next(enc.parameters()).device, n_crop_bank)


def extract_bank_and_query(model: nn.Module, encoder: str, bank_loader: Iterable, query_loader: Iterable, n_crop: int = 1):
    """(g, y_g, q, y_q, valid): ``extract`` of both loaders through encoder 'q' or 'k' of the pretext model in eval mode
    (``frozen_encoder``); only the query side carries crops; valid: the query loader's count of real samples.  What the kNN monitor
    and the linear-probe monitor share."""
    with frozen_encoder(model, encoder) as enc:
        g, y_g = extract_bank(enc, bank_loader, n_crop)
        q, y_q = extract(enc, query_loader, next(enc.parameters()).device, n_crop)
    valid = query_loader.num_valid_samples() if hasattr(query_loader, "num_valid_samples") else q.shape[0]
    return g, y_g, q, y_q, min(int(valid), q.shape[0])


# ---- valid rows, as the cluster and t-SNE modules decide them ------------------------------------------------------------------
def _valid_rows_np(x32: np.ndarray) -> np.ndarray:
    """The fp32 sum of squares of the row is finite and > 0."""
    with np.errstate(all="ignore"):
        ss = (x32 * x32).sum(axis=1, dtype=np.float32)
        return np.isfinite(ss) & (ss > 0)


def _valid_rows_torch(x: Tensor) -> Tensor:
    ss = (x * x).sum(dim=1)
    return torch.isfinite(ss) & (ss > 0)


def _rows(x: Tensor) -> Tensor:
    """x as the fp32 matrix the row kernels take: unit column stride, an even row pitch."""
    x = x.to(torch.float32)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) % 2):
        x = x.contiguous()
    return x


class KNNMonitor(EpochMonitor):
    """Every ``every``-th epoch (and on the last one): weighted kNN accuracy of a labelled query set against a labelled bank on the
    features of one encoder of the pretext model.  ``run`` leaves the model as it found it -- state_dict() bit for bit (eval-mode
    BatchNorm moves no statistics, no queue or counter is touched), every module's ``training`` flag -- draws from no global random
    generator and refuses to run inside a graph capture.  Config, e.g. {"every": 1, "k": 200, "t": 0.07, "num_classes": 101,
    "encoder": "q", "bank_samples": 256, "query_samples": 128, "batch_size": 32, "n_crop": 1}."""

    KEY = "knn_monitor"
    KEYS = ("every", "k", "t", "num_classes", "encoder", "bank_samples", "query_samples", "batch_size", "n_crop")

    def __init__(self, every: int, num_epochs: int, k: int = 200, t: float = 0.07, num_classes: int = 101, encoder: str = "q",
                 bank_samples: int = 256, query_samples: int = 128, batch_size: int = 32, n_crop: int = 1):
        check_limits(k, t, num_classes)
        self._check_encoder(encoder)
        self._check_at_least_1(every=every, bank_samples=bank_samples, query_samples=query_samples, batch_size=batch_size, n_crop=n_crop)
        self.every, self.num_epochs = int(every), int(num_epochs)
        self.k, self.t, self.num_classes, self.encoder = int(k), float(t), int(num_classes), encoder
        self.bank_samples, self.query_samples = int(bank_samples), int(query_samples)
        self.batch_size, self.n_crop = int(batch_size), int(n_crop)

    def build_loaders(self, T: int, size: int, device, seed: int = 0) -> tuple:
        """The stand-in data: two ``SyntheticLabelledClips``, bank = split 'train' (order fixed by its epoch 0), query = split 'val'."""
        return synthetic_loaders(self.bank_samples, self.query_samples, self.batch_size, self.num_classes, self.n_crop, T, size, device, seed)

    def run(self, model: nn.Module, bank_loader: Iterable, query_loader: Iterable, return_features: bool = False) -> dict:
        """{"acc1", "acc5", "n_bank", "n_query", "seconds"}, with ``return_features`` also "bank_features": the (n_bank, D) backbone
        features it extracted, on the device.  ``model``: the pretext model (or its wrapper with ``.module``)."""
        self._refuse_capture()
        t0 = time.perf_counter()
        g, y_g, q, y_q, valid = extract_bank_and_query(model, self.encoder, bank_loader, query_loader, self.n_crop)
        res = knn_classify(q, y_q, g, y_g, self.k, self.t, self.num_classes, valid=valid)
        out = {"acc1": res["acc1"], "acc5": res["acc5"], "n_bank": int(g.shape[0]), "n_query": res["n"],
               "seconds": time.perf_counter() - t0}
        if return_features:
            out["bank_features"] = g
        return out

    def run_epoch(self, model, loaders: tuple, ctx: dict) -> dict:
        """With the representation monitor due as well, the bank's backbone features are left in ctx for it."""
        r = self.run(model, *loaders, **({"return_features": True} if "repr_monitor" in ctx["due"] else {}))
        ctx["bank_features"] = r.pop("bank_features", None)
        return r

    def scalars(self, result: dict) -> dict:
        return {"knn/acc1": result["acc1"], "knn/acc5": result["acc5"]}

    def log_line(self, result: dict, ctx: dict) -> str:
        r = result
        return (f"kNN [{ctx['epoch']}/{ctx['num_epochs']}]\tAcc@1 {r['acc1']:.2f}\tAcc@5 {r['acc5']:.2f}"
                f"\t(k={self.k}, T={self.t}, bank {r['n_bank']}, query {r['n_query']}, {r['seconds']:.1f} s)")


# ---- command line over saved retrieval features --------------------------------------------------------------------------
def classify_features(feature_dir: str, fold: int, k: int = 200, t: float = 0.07, device=None) -> dict:
    """The test features of ``rspnet_amd.retrieval`` against its train features; num_classes = the largest label + 1.  Logs one line
    and writes ``knn_fold{F}.json``."""
    from .retrieval import load_features
    X_train, y_train, X_test, y_test = load_features(feature_dir, fold)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(device)
    num_classes = int(max(y_train.max(), y_test.max())) + 1
    res = knn_classify(torch.as_tensor(X_test, dtype=torch.float32).to(dev).contiguous(), torch.as_tensor(y_test).to(dev),
                       torch.as_tensor(X_train, dtype=torch.float32).to(dev).contiguous(), torch.as_tensor(y_train).to(dev),
                       k=k, T=t, num_classes=num_classes)
    (h1, h5), n = res["hits"], res["n"]
    logger.info("kNN k={} T={}: Acc@1 = {:.2f}% ({}/{}), Acc@5 = {:.2f}% ({}/{})".format(k, t, res["acc1"], h1, n, res["acc5"], h5, n))
    out = {"k": int(k), "t": float(t), "acc1": res["acc1"], "acc5": res["acc5"], "hits1": h1, "hits5": h5, "total": n}
    with open(os.path.join(feature_dir, f"knn_fold{fold}.json"), "w") as fp:
        json.dump(out, fp)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="weighted kNN classification over a directory of saved retrieval features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--t", type=float, default=0.07)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return classify_features(args.features, args.fold, args.k, args.t)


if __name__ == "__main__":
    main()
