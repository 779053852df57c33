"""Linear probe: a softmax classifier fitted on frozen backbone features -- the most quoted read of a self-supervised video
representation, and the one the reference configures (``config/finetune/addition.libsonnet``: ``linear:: {only_train_fc: true}``).
The reference runs the frozen backbone again over every clip on every epoch; here the features are extracted once (``knn.extract``,
or the files ``rspnet_amd.retrieval`` saved) and only the fit runs: on the HIP backend ONE call, rsp_linear_probe_fit
(csrc/linear_probe.hip), issues every step; nothing is read back in between and the learning-rate schedule is a device array.

The rule (include/rspnet_hip.h states it for the kernels; ``probe_reference`` restates it in numpy fp64):

    row factor  f_i = scale / |x_i| (normalize) or scale
    valid rows  the fp32 sum of squares of the row is finite and > 0 (normalize = False: finite), and 0 <= y_i < C.  An invalid row
                takes part in nothing and is counted: counts = (valid rows, invalid rows)
    model       z = (x f) W^T + b, W (C, D) as nn.Linear.weight
    step t      rows [r0, r0 + n), r0 = (t mod ceil(N / batch)) * batch, n = min(batch, N - r0); m = the valid rows among them;
                loss_t = mean over them of logsumexp(z_i) - z_i[y_i] (0 with m = 0); G_i = (softmax(z_i) - onehot(y_i)) / m;
                dW = G^T (x f) + wd W, db = sum_i G_i + wd b; buf = (first_step + t == 0) ? d : mu buf + d; p -= lr[first_step + t] buf

Limits, enforced here with ValueError as the kernel enforces them with RSP_EINVAL: 1 <= C <= 1024, 1 <= N, D even and 2 <= D <= 4096,
1 <= batch <= N, 1 <= steps.

The defaults of ``fit`` (100 steps, full batch, lr 0.125 with a cosine schedule, momentum 0.9, weight decay 1e-4, unit rows scaled by
8) were checked on clustered synthetic inputs only, where the fp64 rule reaches training accuracy 1.0 within 100 full-batch steps.
They are starting points for real features and are tuned on none.

``LinearProbeMonitor`` is the pretext driver's opt-in hook (config key ``probe_monitor``); ``python -m rspnet_amd.linear_probe
--features DIR --fold F`` fits on the train features ``rspnet_amd.retrieval`` saved and evaluates on its test features.  The probe
sees pre-pooled features and no augmentation: a monitor, not a replacement for the reference's ``finetune -x linear``.
"""
from __future__ import annotations

import argparse
import collections
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
from . import knn as _knn
from . import ops as _ops
from .framework.monitor import EpochMonitor

logger = logging.getLogger(__name__)
MAX_CLASSES, MAX_D = 1024, 4096

Probe = collections.namedtuple("Probe", "w b loss_trace counts normalize scale")       # of fit: tensors on x's device
ProbeRef = collections.namedtuple("ProbeRef", "w b mom loss_trace counts logits")       # of probe_reference: numpy fp64


def check_limits(N, D, num_classes, batch, steps):
    """ValueError for values rsp_linear_probe_fit would reject."""
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"linear_probe: num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
    if int(N) < 1:
        raise ValueError(f"linear_probe: at least one row, got {N}")
    if not (2 <= int(D) <= MAX_D and int(D) % 2 == 0):
        raise ValueError(f"linear_probe: D must be even and in [2, {MAX_D}], got {D}")
    if not 1 <= int(batch) <= int(N):
        raise ValueError(f"linear_probe: batch must be in [1, N = {N}], got {batch}")
    if int(steps) < 1:
        raise ValueError(f"linear_probe: steps must be at least 1, got {steps}")


def lr_schedule(lr: float, steps: int, schedule: str = "cosine") -> np.ndarray:
    """The fp32 learning rate of every step: ``lr`` throughout, or ``lr * (1 + cos(pi t / steps)) / 2``."""
    if schedule == "constant":
        return np.full(int(steps), lr, dtype=np.float32)
    if schedule != "cosine":
        raise ValueError(f"linear_probe: schedule must be 'cosine' or 'constant', got {schedule!r}")
    t = np.arange(int(steps), dtype=np.float64)
    return (float(lr) * 0.5 * (1.0 + np.cos(np.pi * t / int(steps)))).astype(np.float32)


def _valid_rows_np(x32: np.ndarray, y, C: int, normalize: bool, labelled: bool = True):
    with np.errstate(all="ignore"):
        ss = (x32 * x32).sum(axis=1, dtype=np.float32)
        ok = np.isfinite(ss) & ((ss > 0) if normalize else True)
    if labelled:
        ok = ok & (y >= 0) & (y < C)
    return ok


# ---- the definition in numpy fp64 ----------------------------------------------------------------------------------------
def reference_logits(w, b, x, normalize: bool = True, scale: float = 8.0) -> np.ndarray:
    """z of the rule in fp64 for the rows of x; NaN in every class of an invalid row (validity without the label condition)."""
    x32 = np.asarray(x, dtype=np.float32)
    w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = _valid_rows_np(x32, None, w.shape[0], normalize, labelled=False)
    a = x32[ok].astype(np.float64)
    a = a * (float(scale) / np.linalg.norm(a, axis=1, keepdims=True)) if normalize else a * float(scale)
    out = np.full((x32.shape[0], w.shape[0]), np.nan)
    out[ok] = a @ w.T + b
    return out


def probe_reference(x, y, num_classes: int, lr, steps: int, batch: Optional[int] = None, momentum: float = 0.9,
                    weight_decay: float = 1e-4, normalize: bool = True, scale: float = 8.0, w0=None, b0=None, mom0=None,
                    first_step: int = 0, x2=None) -> ProbeRef:
    """The rule of the module docstring in numpy fp64 (validity is decided on the fp32 sum of squares, as the kernel decides it).
    lr: one learning rate per step, indexed by first_step + t.  w0 / b0 / mom0: the state the fit starts from (zeros by default).
    Returns (w, b, mom (C * D + C,), loss_trace, counts, logits of the rows of ``x2`` -- NaN rows for its invalid ones -- or None)."""
    x32 = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.int64).reshape(-1)
    N, D = x32.shape
    C = int(num_classes)
    batch = N if batch is None else int(batch)
    lr = np.asarray(lr, dtype=np.float64)
    mu, wd, scale = float(momentum), float(weight_decay), float(scale)

    def hat(a32, ok):
        a = a32[ok].astype(np.float64)
        return a * (scale / np.linalg.norm(a, axis=1, keepdims=True)) if normalize else a * scale

    ok = _valid_rows_np(x32, y, C, normalize)
    W = np.zeros((C, D)) if w0 is None else np.array(w0, dtype=np.float64)
    b = np.zeros(C) if b0 is None else np.array(b0, dtype=np.float64)
    mom = np.zeros(C * D + C) if mom0 is None else np.array(mom0, dtype=np.float64).reshape(-1)
    mW, mb = mom[:C * D].reshape(C, D).copy(), mom[C * D:].copy()
    nchunks = -(-N // batch)
    trace = np.zeros(int(steps))
    for t in range(int(steps)):
        r0 = (t % nchunks) * batch
        sl = slice(r0, min(r0 + batch, N))
        xh, yy = hat(x32[sl], ok[sl]), y[sl][ok[sl]]
        m = xh.shape[0]
        if m:
            z = xh @ W.T + b
            zmax = z.max(axis=1, keepdims=True)
            e = np.exp(z - zmax)
            ssum = e.sum(axis=1, keepdims=True)
            trace[t] = ((zmax[:, 0] + np.log(ssum[:, 0])) - z[np.arange(m), yy]).mean()
            G = e / ssum
            G[np.arange(m), yy] -= 1.0
            G /= m
            dW, db = G.T @ xh + wd * W, G.sum(axis=0) + wd * b
        else:
            dW, db = wd * W, wd * b
        step = int(first_step) + t
        mW, mb = (dW, db) if step == 0 else (mu * mW + dW, mu * mb + db)
        W, b = W - lr[step] * mW, b - lr[step] * mb
    logits = None if x2 is None else reference_logits(W, b, x2, normalize, scale)
    return ProbeRef(W, b, np.concatenate([mW.reshape(-1), mb]), trace, (int(ok.sum()), int(N - ok.sum())), logits)


# ---- the same rule from torch ops ----------------------------------------------------------------------------------------
def _rows_torch(x: Tensor, y: Optional[Tensor], C: int, normalize: bool, scale: float):
    """(x f with the invalid rows dropped, their labels, the flags)."""
    ss = (x * x).sum(dim=1)
    ok = torch.isfinite(ss) & ((ss > 0) if normalize else torch.ones_like(ss, dtype=torch.bool))
    if y is not None:
        ok = ok & (y >= 0) & (y < C)
    keep = ok.nonzero().reshape(-1)
    xk = x.index_select(0, keep)
    f = (scale / xk.norm(dim=1, keepdim=True)) if normalize else scale
    return xk * f, (y.index_select(0, keep) if y is not None else None), ok


def _probe_torch(x: Tensor, y: Tensor, w: Tensor, b: Tensor, mom: Tensor, lr: Tensor, steps: int, batch: int, first_step: int = 0,
                 momentum: float = 0.9, weight_decay: float = 1e-4, normalize: bool = True, scale: float = 8.0):
    """The rule from torch ops on whatever device the tensors are on; w, b and mom change in place.  Returns (loss_trace, counts).  The
    invalid rows are dropped chunk by chunk before anything is multiplied (a host round trip per chunk: this is the fallback)."""
    N, D = x.shape
    C = w.shape[0]
    nchunks = -(-N // batch)
    chunks, valid = [], 0
    for c in range(nchunks):
        sl = slice(c * batch, min((c + 1) * batch, N))
        xh, yy, ok = _rows_torch(x[sl], y[sl], C, normalize, scale)
        chunks.append((xh, yy))
        valid += int(ok.sum())
    mW, mb = mom[:C * D].view(C, D), mom[C * D:]
    trace = torch.zeros(steps, dtype=torch.float32, device=x.device)
    for t in range(steps):
        xh, yy = chunks[t % nchunks]
        m = xh.shape[0]
        if m:
            z = xh @ w.t() + b
            zmax = z.max(dim=1, keepdim=True).values
            e = torch.exp(z - zmax)
            ssum = e.sum(dim=1, keepdim=True)
            trace[t] = ((zmax[:, 0] + torch.log(ssum[:, 0])) - z.gather(1, yy[:, None])[:, 0]).mean()
            G = e / ssum
            G.scatter_add_(1, yy[:, None], torch.full((m, 1), -1.0, dtype=G.dtype, device=G.device))
            G = G / m
            dW, db = G.t() @ xh + weight_decay * w, G.sum(dim=0) + weight_decay * b
        else:
            dW, db = weight_decay * w, weight_decay * b
        step = first_step + t
        if step == 0:
            mW.copy_(dW)
            mb.copy_(db)
        else:
            mW.mul_(momentum).add_(dW)
            mb.mul_(momentum).add_(db)
        w.sub_(lr[step] * mW)
        b.sub_(lr[step] * mb)
    return trace, torch.tensor([valid, N - valid], dtype=torch.int32, device=x.device)


def _logits_torch(x: Tensor, w: Tensor, b: Tensor, normalize: bool, scale: float) -> Tensor:
    xh, _, ok = _rows_torch(x, None, w.shape[0], normalize, scale)
    out = torch.full((x.shape[0], w.shape[0]), float("nan"), dtype=torch.float32, device=x.device)
    out[ok] = xh @ w.t() + b
    return out


# ---- the public calls ----------------------------------------------------------------------------------------------------
def fit_raw(x: Tensor, y: Tensor, w: Tensor, b: Tensor, mom: Tensor, lr: Tensor, steps: int, batch: Optional[int] = None,
            first_step: int = 0, momentum: float = 0.9, weight_decay: float = 1e-4, normalize: bool = True, scale: float = 8.0):
    """``steps`` steps from the state (w, b, mom), which changes in place, on the rows of x in their order: one rsp_linear_probe_fit
    call when the active op backend has ``linear_probe_fit``, the same rule from torch ops otherwise.  (loss_trace, counts)."""
    N, D = x.shape
    batch = N if batch is None else int(batch)
    check_limits(N, D, w.shape[0], batch, steps)
    if int(first_step) < 0 or lr.numel() < int(first_step) + int(steps):
        raise ValueError(f"linear_probe: {lr.numel()} learning rates for steps {first_step} .. {int(first_step) + int(steps)}")
    kw = dict(first_step=int(first_step), momentum=float(momentum), weight_decay=float(weight_decay), normalize=bool(normalize),
              scale=float(scale))
    be = _ops.backend()
    if hasattr(be, "linear_probe_fit"):
        return be.linear_probe_fit(x, y, w, b, mom, lr, int(steps), batch, **kw)
    return _probe_torch(x, y, w, b, mom, lr, int(steps), batch, **kw)


def fit(x: Tensor, y: Tensor, num_classes: int, steps: int = 100, batch: Optional[int] = None, lr: float = 0.125,
        schedule: str = "cosine", momentum: float = 0.9, weight_decay: float = 1e-4, normalize: bool = True, scale: float = 8.0,
        seed: int = 0) -> Probe:
    """Fit the probe from zeros on the rows of x (N, D) with labels y.  With batch < N the rows are shuffled once, by a generator of
    this call's own seeded with ``seed`` (no global generator is drawn from).  Returns Probe(w, b, loss_trace, counts, ...)."""
    N, D = x.shape
    batch = N if batch is None else int(batch)
    check_limits(N, D, num_classes, batch, steps)
    x = x.to(torch.float32)
    y = y.to(torch.int64).reshape(-1)
    if batch < N:
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed))).to(x.device)
        x, y = x.index_select(0, perm), y.index_select(0, perm)
    if x.stride(1) != 1 or (N > 1 and x.stride(0) % 2):
        x = x.contiguous()
    y = y.contiguous()
    C, dev = int(num_classes), x.device
    w = torch.zeros((C, D), dtype=torch.float32, device=dev)
    b = torch.zeros(C, dtype=torch.float32, device=dev)
    mom = torch.zeros(C * D + C, dtype=torch.float32, device=dev)
    lr_dev = torch.from_numpy(lr_schedule(lr, steps, schedule)).to(dev)
    trace, counts = fit_raw(x, y, w, b, mom, lr_dev, steps, batch, 0, momentum, weight_decay, normalize, scale)
    return Probe(w, b, trace, counts, bool(normalize), float(scale))


def logits(probe: Probe, x: Tensor) -> Tensor:
    """(N, C) logits of the rows of x; NaN in every class of an invalid row."""
    x = x.to(torch.float32)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) % 2):
        x = x.contiguous()
    be = _ops.backend()
    if hasattr(be, "linear_probe_logits"):
        return be.linear_probe_logits(x, probe.w, probe.b, probe.normalize, probe.scale)
    return _logits_torch(x, probe.w, probe.b, probe.normalize, probe.scale)


def evaluate(probe: Probe, x: Tensor, y: Tensor, valid: Optional[int] = None) -> dict:
    """{"loss", "acc1", "acc5" (percent over the first ``valid`` rows), "hits" (hits1, hits5), "n", "pred", "rank"} of the probe on
    the rows of x with labels y: the logits, then the fine-tune driver's metrics (rsp_xent_metrics on the HIP backend: an invalid
    row's NaN logits count as a miss; a label outside [0, C) is a miss as well)."""
    N, C = x.shape[0], probe.w.shape[0]
    n = N if valid is None else int(valid)
    if not 0 <= n <= N:
        raise ValueError(f"linear_probe: valid must be in [0, {N}], got {valid}")
    z = logits(probe, x)
    y = y.to(torch.int64).reshape(-1).contiguous()
    good = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    rank = torch.where(good, _ft.rank_of_target(torch.where(z == z, z, torch.full_like(z, -math.inf)), yc), torch.full_like(y, C))
    rank = torch.where(torch.isnan(z).any(dim=1), torch.full_like(rank, C), rank)
    be = _ops.backend()
    if hasattr(be, "xent_metrics") and z.is_cuda and bool(good.all()):
        _, loss, _, _ = be.xent_metrics(z, y, n_crop=1, valid=n, want_grad=False)
        loss = float(loss)      # (its accuracies are fp32 percentages: the integer hit counts come from the ranks, the same tie rule)
    else:
        zz, tt = z[:n][good[:n]], y[:n][good[:n]]
        loss = float(torch.nn.functional.cross_entropy(zz, tt)) if zz.shape[0] else 0.0
    h1, h5 = int((rank[:n] < 1).sum()), int((rank[:n] < 5).sum())
    return {"loss": loss, "acc1": 100.0 * h1 / n if n else 0.0, "acc5": 100.0 * h5 / n if n else 0.0, "hits": (h1, h5), "n": n,
            "pred": z.argmax(dim=1), "rank": rank}


# ---- the pretext driver's hook -------------------------------------------------------------------------------------------
class LinearProbeMonitor(EpochMonitor):
    """Every ``every``-th epoch (and on the last one): a probe fitted on the backbone features of a labelled bank and evaluated on
    those of a labelled query set, both from one encoder of the pretext model (``knn.extract``).  ``run`` leaves the model as it
    found it -- state_dict() bit for bit, every module's ``training`` flag --, draws from no global random generator and refuses to
    run inside a graph capture.  The extraction and the stand-in loaders are the kNN monitor's (``knn.extract_bank_and_query``,
    ``knn.synthetic_loaders``); each monitor still extracts for itself, since ``KNNMonitor.run`` hands back the bank's features only.
    Config, e.g. {"every": 10, "num_classes": 101, "steps": 100, "lr": 0.125}."""

    KEY = "probe_monitor"
    KEYS = ("every", "num_classes", "encoder", "bank_samples", "query_samples", "batch_size", "n_crop", "steps", "lr", "momentum",
            "weight_decay", "scale", "batch")

    def __init__(self, every: int, num_epochs: int, num_classes: int = 101, encoder: str = "q", bank_samples: int = 256,
                 query_samples: int = 128, batch_size: int = 32, n_crop: int = 1, steps: int = 100, lr: float = 0.125,
                 momentum: float = 0.9, weight_decay: float = 1e-4, scale: float = 8.0, batch: Optional[int] = None):
        self._check_encoder(encoder)
        self._check_at_least_1(every=every, bank_samples=bank_samples, query_samples=query_samples, batch_size=batch_size, n_crop=n_crop)
        check_limits(bank_samples, 2, num_classes, bank_samples if batch is None else batch, steps)
        self.every, self.num_epochs = int(every), int(num_epochs)
        self.num_classes, self.encoder = int(num_classes), encoder
        self.bank_samples, self.query_samples = int(bank_samples), int(query_samples)
        self.batch_size, self.n_crop = int(batch_size), int(n_crop)
        self.steps, self.lr, self.momentum, self.weight_decay = int(steps), float(lr), float(momentum), float(weight_decay)
        self.scale, self.batch = float(scale), None if batch is None else int(batch)

    def build_loaders(self, T: int, size: int, device, seed: int = 0) -> tuple:
        """The stand-in data of the kNN monitor: bank = split 'train', query = split 'val' of ``SyntheticLabelledClips``."""
        return _knn.synthetic_loaders(self.bank_samples, self.query_samples, self.batch_size, self.num_classes, self.n_crop, T, size, device,
                                      seed)

    def run(self, model: nn.Module, bank_loader: Iterable, query_loader: Iterable) -> dict:
        """{"acc1", "acc5", "loss", "train_loss", "n_bank", "n_query", "bad_rows", "seconds"}."""
        self._refuse_capture()
        t0 = time.perf_counter()
        g, y_g, q, y_q, valid = _knn.extract_bank_and_query(model, self.encoder, bank_loader, query_loader, self.n_crop)
        with torch.no_grad():
            batch = None if self.batch is None else min(self.batch, g.shape[0])
            probe = fit(g, y_g, self.num_classes, steps=self.steps, batch=batch, lr=self.lr, momentum=self.momentum,
                        weight_decay=self.weight_decay, scale=self.scale)
            res = evaluate(probe, q, y_q, valid=valid)
        return {"acc1": res["acc1"], "acc5": res["acc5"], "loss": res["loss"], "train_loss": float(probe.loss_trace[-1]),
                "n_bank": int(g.shape[0]), "n_query": res["n"], "bad_rows": int(probe.counts[1]), "seconds": time.perf_counter() - t0}

    def scalars(self, result: dict) -> dict:
        return {f"probe_{k}": result[k] for k in ("acc1", "acc5", "loss")}

    def log_line(self, result: dict, ctx: dict) -> str:
        r = result
        return (f"Probe [{ctx['epoch']}/{ctx['num_epochs']}]\tAcc@1 {r['acc1']:.2f}\tAcc@5 {r['acc5']:.2f}\tloss {r['loss']:.4f}"
                f"\t({self.steps} steps, lr {self.lr}, bank {r['n_bank']}, query {r['n_query']}, {r['bad_rows']} bad, "
                f"{r['seconds']:.1f} s)")


# ---- command line over saved retrieval features --------------------------------------------------------------------------
def probe_features(feature_dir: str, fold: int, steps: int = 100, batch: Optional[int] = None, lr: float = 0.125, wd: float = 1e-4,
                   scale: float = 8.0, normalize: bool = True, device=None) -> dict:
    """Fit on the train features ``rspnet_amd.retrieval`` saved, evaluate on its test features; num_classes = the largest label + 1.
    Logs one line and writes ``probe_fold{F}.json``."""
    from .retrieval import load_features
    X_train, y_train, X_test, y_test = load_features(feature_dir, fold)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(device)
    num_classes = int(max(y_train.max(), y_test.max())) + 1
    probe = fit(torch.as_tensor(X_train, dtype=torch.float32).to(dev).contiguous(), torch.as_tensor(y_train).to(dev), num_classes,
                steps=steps, batch=batch, lr=lr, weight_decay=wd, normalize=normalize, scale=scale)
    res = evaluate(probe, torch.as_tensor(X_test, dtype=torch.float32).to(dev).contiguous(), torch.as_tensor(y_test).to(dev))
    (h1, h5), n = res["hits"], res["n"]
    logger.info("Linear probe steps={} lr={}: Acc@1 = {:.2f}% ({}/{}), Acc@5 = {:.2f}% ({}/{}), loss {:.4f}".format(
        steps, lr, res["acc1"], h1, n, res["acc5"], h5, n, res["loss"]))
    out = {"steps": int(steps), "batch": None if batch is None else int(batch), "lr": float(lr), "weight_decay": float(wd),
           "scale": float(scale), "normalize": bool(normalize), "acc1": res["acc1"], "acc5": res["acc5"], "loss": res["loss"],
           "hits1": h1, "hits5": h5, "total": n, "train_loss": float(probe.loss_trace[-1]), "bad_rows": int(probe.counts[1])}
    with open(os.path.join(feature_dir, f"probe_fold{fold}.json"), "w") as fp:
        json.dump(out, fp)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="linear probe over a directory of saved retrieval features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=None, help="rows per step (default: all)")
    ap.add_argument("--lr", type=float, default=0.125)
    ap.add_argument("--wd", type=float, default=1e-4)
    ap.add_argument("--scale", type=float, default=8.0)
    ap.add_argument("--no-normalize", action="store_true")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return probe_features(args.features, args.fold, args.steps, args.batch, args.lr, args.wd, args.scale, not args.no_normalize)


if __name__ == "__main__":
    main()
