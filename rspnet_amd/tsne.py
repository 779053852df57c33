"""Embedding maps: exact t-SNE of frozen features, the 2-D neighbour-embedding picture of a self-supervised representation coloured by
class.  On the HIP backend the affinities are ONE call (rsp_tsne_affinities) and the whole descent is ONE call (rsp_tsne_fit,
csrc/tsne.hip): the low-dimensional N x N matrices are never stored and nothing is read back between iterations.

The rule (include/rspnet_hip.h states it for the kernels; ``tsne_reference`` restates it in numpy fp64):

    valid rows   the fp32 sum of squares of the row is finite and > 0; the valid rows are listed in ascending order (M of them) and an
                 invalid row takes part in nothing: the result is the result on x without it
    distance     d_ij = max(2 - 2 s_ij, 0) with the cosine similarity s of the search
    calibration  per row, over j != i: m = min_j d_ij, e_j(b) = exp(-b (d_ij - m)), S = sum e, A = sum e (d - m), H = log S + b A / S;
                 b = 1, lo = 0, hi = inf, then exactly 64 steps: H > log(perplexity): lo = b, b = 2 b while hi is inf, else the mid-point;
                 otherwise hi = b, b = the mid-point.  c_ij = e_j(beta_i) / S_i
    joint        p_ij = (c_ij + c_ji) / (2 M), p_ii = 0
    iteration    w = 1 / (1 + |y_i - y_j|^2); attr_i = sum p w (y_i - y_j), rep_i = sum w^2 (y_i - y_j), Z = sum_{i != j} w,
                 E = sum p log1p(r2); g = 4 (exag attr - rep / Z); kl = plogp + E + log Z (before the update, un-exaggerated p);
                 gains = gains + 0.2 where sign(g) != sign(inc) else gains * 0.8, floored at 0.01; inc = mom inc - lr gains g; y += inc

Limits, enforced here with ValueError as the kernels enforce them with RSP_EINVAL: 2 <= N <= 16384, D even and 2 <= D <= 4096,
perplexity finite and in [1, 1024], 1 <= iters <= 10000.

``TsneMonitor`` is the pretext driver's opt-in hook (config key ``tsne_monitor``); ``python -m rspnet_amd.tsne --features DIR --fold F``
maps the features ``rspnet_amd.retrieval`` saved.  The monitor has run on one GPU only.
"""
from __future__ import annotations

import argparse
import collections
import colorsys
import json
import logging
import math
import os
import time
from typing import Iterable, Optional

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib
from . import knn as _knn
from . import ops as _ops
from .framework.monitor import EpochMonitor
from .knn import _rows, _valid_rows_np, _valid_rows_torch

logger = logging.getLogger(__name__)
MAX_ROWS, MAX_D, MAX_PERPLEXITY, MAX_ITERS, CALIB_STEPS = 16384, 4096, 1024.0, 10000, 64

Tsne = collections.namedtuple("Tsne", "y kl_trace beta info")                       # of fit
Affinities = collections.namedtuple("Affinities", "rows d beta p plogp psum")      # of affinities_reference: numpy fp64, M x M
INFO_KEYS = ("plogp", "psum", "rows_valid", "rows_bad")


def check_limits(N, D, perplexity=30.0, iters=1):
    """ValueError for values rsp_tsne_affinities / rsp_tsne_fit would reject."""
    if not 2 <= int(N) <= MAX_ROWS:
        raise ValueError(f"tsne: N must be in [2, {MAX_ROWS}], got {N}")
    if not (2 <= int(D) <= MAX_D and int(D) % 2 == 0):
        raise ValueError(f"tsne: D must be even and in [2, {MAX_D}], got {D}")
    if not (math.isfinite(float(perplexity)) and 1.0 <= float(perplexity) <= MAX_PERPLEXITY):
        raise ValueError(f"tsne: perplexity must be finite and in [1, {MAX_PERPLEXITY:g}], got {perplexity}")
    if not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"tsne: iters must be in [1, {MAX_ITERS}], got {iters}")


def schedule(iters: int, lr: float, exag: float = 12.0, exag_iters: int = 250, mom_early: float = 0.5, mom_late: float = 0.8) -> np.ndarray:
    """(iters, 4) fp32: lr, momentum, exaggeration and a pad word per iteration."""
    s = np.zeros((int(iters), 4), dtype=np.float32)
    s[:, 0] = lr
    s[:, 1] = np.where(np.arange(int(iters)) < int(exag_iters), mom_early, mom_late)
    s[:, 2] = np.where(np.arange(int(iters)) < int(exag_iters), exag, 1.0)
    return s


# ---- the definition in numpy fp64 ----------------------------------------------------------------------------------------
def reference_distances(x) -> tuple:
    """(rows, d): the list of valid rows and the M x M fp64 distances of the rule (diagonal 0)."""
    x32 = np.asarray(x, dtype=np.float32)
    rows = np.flatnonzero(_valid_rows_np(x32))
    a = x32[rows].astype(np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    d = np.maximum(2.0 - 2.0 * (a @ a.T), 0.0)
    np.fill_diagonal(d, 0.0)
    return rows, d


def calibrate(d, perplexity: float, dtype=np.float64):
    """(beta, cond) of the rule on an M x M distance matrix, every row at once; dtype = np.float32 gives the fp32 restatement."""
    d = np.asarray(d, dtype=dtype)
    M = d.shape[0]
    off = ~np.eye(M, dtype=bool)
    m = np.where(off, d, np.inf).min(axis=1)
    dd = np.where(off, d - m[:, None], 0).astype(dtype)
    logp = dtype(np.log(dtype(perplexity)))
    beta, lo, hi = np.ones(M, dtype), np.zeros(M, dtype), np.full(M, np.inf, dtype)
    for _ in range(CALIB_STEPS):
        e = np.where(off, np.exp(-beta[:, None] * dd), 0).astype(dtype)
        S, A = e.sum(axis=1), (e * dd).sum(axis=1)
        with np.errstate(all="ignore"):
            up = (np.log(S) + beta * A / S) > logp
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        with np.errstate(all="ignore"):
            beta = np.where(up & np.isinf(hi), dtype(2) * beta, (lo + hi) / dtype(2)).astype(dtype)
    e = np.where(off, np.exp(-beta[:, None] * dd), 0).astype(dtype)
    return beta, e / e.sum(axis=1, keepdims=True)


def joint(cond):
    M = cond.shape[0]
    p = (cond + cond.T) * (cond.dtype.type(1) / cond.dtype.type(2 * M))
    np.fill_diagonal(p, 0)
    return p


def affinities_reference(x=None, perplexity: float = 30.0, d=None, rows=None) -> Affinities:
    """The affinities of the rule in fp64, from x or -- to follow a kernel's own distances -- from a given M x M matrix d."""
    if d is None:
        rows, d = reference_distances(x)
    d = np.asarray(d, dtype=np.float64)
    beta, cond = calibrate(d, perplexity)
    p = joint(cond)
    pos = p[p > 0]
    return Affinities(rows, d, beta, p, float((pos * np.log(pos)).sum()), float(p.sum()))


def step_reference(p, plogp, y, inc, gains, lr, mom, exag):
    """One iteration of the rule in the arrays' dtype (fp64 for the reference): (g, y, inc, gains, kl) with kl of the map before the update."""
    dt = y.dtype.type
    diff = y[:, None, :] - y[None, :, :]
    r2 = (diff * diff).sum(axis=2)
    w = dt(1) / (dt(1) + r2)
    np.fill_diagonal(w, 0)
    attr = ((p * w)[:, :, None] * diff).sum(axis=1)
    rep = ((w * w)[:, :, None] * diff).sum(axis=1)
    Z = w.sum(dtype=np.float64)
    E = (p * np.log1p(r2)).sum(dtype=np.float64)
    with np.errstate(all="ignore"):
        g = dt(4) * (dt(exag) * attr - rep / dt(Z))
        kl = float(plogp + E + np.log(Z))
    gains = np.maximum(np.where((g > 0) != (inc > 0), gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    inc = dt(mom) * inc - dt(lr) * gains * g
    return g, y + inc, inc, gains, kl


TsneRef = collections.namedtuple("TsneRef", "aff y inc gains kl states grads")


def tsne_reference(x, perplexity, sched, y0, iters: int, keep=(), aff: Optional[Affinities] = None) -> TsneRef:
    """The whole rule in numpy fp64 on the valid rows of x from y0 (N, 2): states[t] = (y, inc, gains) before iteration t and
    grads[t] = its gradient for t in ``keep``.  y, inc, gains come back over the M listed rows."""
    if aff is None:
        aff = affinities_reference(x, perplexity)
    y = np.asarray(y0, dtype=np.float64)[aff.rows].copy()
    inc, gains = np.zeros_like(y), np.ones_like(y)
    kl, states, grads = np.zeros(int(iters)), {}, {}
    for t in range(int(iters)):
        if t in keep:
            states[t] = (y.copy(), inc.copy(), gains.copy())
        lr, mom, ex = (float(v) for v in sched[t][:3])
        g, y, inc, gains, kl[t] = step_reference(aff.p, aff.plogp, y, inc, gains, lr, mom, ex)
        if t in keep:
            grads[t] = g
    return TsneRef(aff, y, inc, gains, kl, states, grads)


# ---- the same rule from torch ops (any device; stores the M x M matrices: this is what a backend without the entry points runs) --
def affinities_torch(x: Tensor, perplexity: float):
    """(rows int64 (M,), d, beta, p, plogp, psum) in fp32 torch ops on x's device."""
    rows = torch.nonzero(_valid_rows_torch(x)).reshape(-1)
    a = x.index_select(0, rows)
    inv = 1.0 / a.norm(dim=1)
    d = torch.clamp(2.0 - 2.0 * ((a @ a.t()) * inv[:, None] * inv[None, :]), min=0.0)
    M = a.shape[0]
    eye = torch.eye(M, dtype=torch.bool, device=x.device)
    d = d.masked_fill(eye, 0.0)
    m = d.masked_fill(eye, math.inf).min(dim=1).values
    dd = (d - m[:, None]).masked_fill(eye, 0.0)
    logp = math.log(perplexity)
    beta, lo = torch.ones(M, device=x.device), torch.zeros(M, device=x.device)
    hi = torch.full((M,), math.inf, device=x.device)
    for _ in range(CALIB_STEPS):
        e = torch.exp(-beta[:, None] * dd).masked_fill(eye, 0.0)
        S, A = e.sum(dim=1), (e * dd).sum(dim=1)
        up = (torch.log(S) + beta * A / S) > logp
        lo = torch.where(up, beta, lo)
        hi = torch.where(up, hi, beta)
        beta = torch.where(up & torch.isinf(hi), 2.0 * beta, (lo + hi) * 0.5)
    e = torch.exp(-beta[:, None] * dd).masked_fill(eye, 0.0)
    cond = e / e.sum(dim=1, keepdim=True)
    p = ((cond + cond.t()) * (1.0 / (2.0 * M))).masked_fill(eye, 0.0)
    p64 = p.to(torch.float64)
    plogp = float((p64 * torch.log(p.clamp_min(1e-45)).to(torch.float64)).sum())
    return rows, d, beta, p, plogp, float(p64.sum())


def step_torch(p: Tensor, plogp: float, y: Tensor, inc: Tensor, gains: Tensor, lr: float, mom: float, exag: float):
    """One iteration of the rule from fp32 torch ops, y / inc / gains (M, 2) updated in place; returns (g, kl as a 0-d fp64 tensor)."""
    diff = y[:, None, :] - y[None, :, :]
    r2 = (diff * diff).sum(dim=2)
    w = 1.0 / (1.0 + r2)
    w.fill_diagonal_(0.0)
    attr = ((p * w)[:, :, None] * diff).sum(dim=1)
    rep = ((w * w)[:, :, None] * diff).sum(dim=1)
    Z = w.sum(dtype=torch.float64)
    E = (p * torch.log1p(r2)).sum(dtype=torch.float64)
    g = 4.0 * (exag * attr - rep / Z.to(torch.float32))
    gains.copy_(torch.where((g > 0) != (inc > 0), gains + 0.2, gains * 0.8).clamp_min(0.01))
    inc.mul_(mom).sub_(lr * gains * g)
    y.add_(inc)
    return g, plogp + E + torch.log(Z)


# ---- the public calls ----------------------------------------------------------------------------------------------------
def read_info(info: Tensor) -> dict:
    """The 32-byte rsp_tsne_info of HipOps.tsne_affinities as a dict (one small copy to the host)."""
    rec = _lib.TsneInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return {"plogp": float(rec.plogp), "psum": float(rec.psum), "rows_valid": int(rec.rows_valid), "rows_bad": int(rec.rows_bad)}


def initial_map(x: Tensor, seed: int = 0, init: str = "random") -> Tensor:
    """y0 (N, 2) fp32 on the host: N(0, 1e-4^2) from a CPU generator of the call's own (no global generator is touched), or the
    first two principal components of the valid rows scaled to that spread."""
    N = x.shape[0]
    if init == "random":
        return torch.randn(N, 2, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32) * 1e-4
    if init != "pca":
        raise ValueError(f"tsne: init must be 'random' or 'pca', got {init!r}")
    xc = x.detach().to("cpu", torch.float64)
    ok = _valid_rows_torch(xc.to(torch.float32))
    a = xc[ok] / xc[ok].norm(dim=1, keepdim=True)
    a = a - a.mean(dim=0, keepdim=True)
    _, _, vh = torch.linalg.svd(a, full_matrices=False)
    pc = a @ vh[:2].t() if vh.shape[0] >= 2 else torch.cat([a @ vh[:1].t(), torch.zeros(a.shape[0], 1, dtype=a.dtype)], 1)
    y0 = torch.zeros(N, 2, dtype=torch.float32)
    y0[ok] = (pc / pc[:, 0].std().clamp_min(1e-30) * 1e-4).to(torch.float32)
    return y0


def fit(x: Tensor, perplexity: float = 30.0, iters: int = 1000, exag: float = 12.0, exag_iters: int = 250, lr="auto", seed: int = 0,
        init: str = "random") -> Tsne:
    """The t-SNE map of the rows of x (N, D).  Returns Tsne(y (N, 2) centred over the valid rows, NaN in an invalid row; kl_trace
    fp64 (iters,); beta (N,) by row, NaN in an invalid row; info dict).  lr="auto": max(M / exag / 4, 50); momentum 0.5 during the
    exaggeration and 0.8 after it.  On a backend with ``tsne_affinities`` / ``tsne_fit`` two HIP calls, the same rule from torch
    ops otherwise."""
    N, D = x.shape
    check_limits(N, D, perplexity, iters)
    x = _rows(x)
    dev = x.device
    y0 = initial_map(x, seed, init).to(dev)
    be = _ops.backend()
    hip = hasattr(be, "tsne_affinities") and hasattr(be, "tsne_fit")
    if hip:
        aff = be.tsne_affinities(x, float(perplexity))
        info = read_info(aff.info)
        rows, beta_r = aff.rows[:info["rows_valid"]].to(torch.int64), aff.beta
    else:
        rows, _, beta_r, p, plogp, psum = affinities_torch(x, float(perplexity))
        info = {"plogp": plogp, "psum": psum, "rows_valid": int(rows.numel()), "rows_bad": N - int(rows.numel())}
    M = info["rows_valid"]
    rate = max(M / float(exag) / 4.0, 50.0) if lr == "auto" else float(lr)
    sched = schedule(iters, rate, exag, exag_iters)
    y, inc, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    if hip:
        kl = be.tsne_fit(aff, torch.from_numpy(sched).to(dev), 0, int(iters), y, inc, gains)
        ym = y.index_select(0, rows)
    else:
        ym, im, gm = y.index_select(0, rows), inc.index_select(0, rows), gains.index_select(0, rows)
        kls = [step_torch(p, plogp, ym, im, gm, *(float(v) for v in sched[t][:3]))[1] for t in range(int(iters))]
        kl = torch.stack(kls)
    out = torch.full((N, 2), math.nan, dtype=torch.float32, device=dev)
    beta = torch.full((N,), math.nan, dtype=torch.float32, device=dev)
    if M:
        out[rows] = ym - ym.mean(dim=0, keepdim=True)
        beta[rows] = beta_r[:M]
    return Tsne(out, kl, beta, info)


def neighbour_purity(y, labels, k: int = 10) -> float:
    """The mean, over the rows of the map that are finite, of the share of a row's k nearest rows in the map that carry its label."""
    y = np.asarray(y.cpu() if isinstance(y, Tensor) else y, dtype=np.float64)
    lab = np.asarray(labels.cpu() if isinstance(labels, Tensor) else labels).reshape(-1)
    ok = np.isfinite(y).all(axis=1)
    y, lab = y[ok], lab[ok]
    n = y.shape[0]
    k = min(int(k), n - 1)
    if k < 1:
        return 0.0
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2) if n <= 4096 else None
    if d is None:      # blocks of rows: the full matrix would be large
        hits = 0.0
        for s in range(0, n, 1024):
            blk = ((y[s:s + 1024, None, :] - y[None, :, :]) ** 2).sum(axis=2)
            blk[np.arange(blk.shape[0]), np.arange(s, s + blk.shape[0])] = np.inf
            nn_ = np.argpartition(blk, k - 1, axis=1)[:, :k]
            hits += (lab[nn_] == lab[s:s + 1024, None]).mean(axis=1).sum()
        return float(hits / n)
    np.fill_diagonal(d, np.inf)
    nn_ = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((lab[nn_] == lab[:, None]).mean())


def palette(num_classes: int):
    """A fixed hue per class: class c of n gets hue c / n at full saturation, the value alternating between two levels."""
    n = max(int(num_classes), 1)
    return [tuple(int(round(255 * v)) for v in colorsys.hsv_to_rgb(c / n, 0.85, 1.0 if c % 2 == 0 else 0.7)) for c in range(n)]


def draw(y, labels, size: int = 512):
    """The map as a size x size PIL image on white: one dot per finite row, coloured by ``palette``; the axes share one scale."""
    from PIL import Image, ImageDraw
    y = np.asarray(y.cpu() if isinstance(y, Tensor) else y, dtype=np.float64)
    lab = np.asarray(labels.cpu() if isinstance(labels, Tensor) else labels).reshape(-1).astype(np.int64)
    img = Image.new("RGB", (int(size), int(size)), (255, 255, 255))
    ok = np.isfinite(y).all(axis=1)
    if not ok.any():
        return img
    pts, lab = y[ok], lab[ok]
    colours = palette(int(lab.max()) + 1 if lab.size else 1)
    centre = (pts.max(axis=0) + pts.min(axis=0)) / 2
    span = max(float((pts.max(axis=0) - pts.min(axis=0)).max()), 1e-30)
    margin, r = 0.04 * size, max(1, int(size) // 256)
    xy = (pts - centre) / span * (size - 2 * margin) + size / 2
    pen = ImageDraw.Draw(img)
    for (px, py), c in zip(xy, lab):
        pen.ellipse([px - r, py - r, px + r, py + r], fill=colours[c] if c >= 0 else (0, 0, 0))
    return img


# ---- the pretext driver's hook -------------------------------------------------------------------------------------------
class TsneMonitor(EpochMonitor):
    """Every ``every``-th epoch (and on the last one): the t-SNE map of the backbone features of a labelled bank from one encoder of the
    pretext model (``knn.extract``), written as ``tsne_epoch{E}.png`` / ``.npy``, with its final KL and its neighbour purity.  ``run``
    leaves the model as it found it -- state_dict() bit for bit, every module's ``training`` flag --, draws from no global random
    generator and refuses to run inside a graph capture.  Has run on one GPU only.  Config, e.g. {"every": 10, "perplexity": 30,
    "iters": 500}."""

    KEY = "tsne_monitor"
    KEYS = ("every", "perplexity", "iters", "encoder", "bank_samples", "batch_size", "n_crop", "seed")
    NUM_CLASSES = 10      # of the stand-in bank

    def __init__(self, every: int, num_epochs: int, perplexity: float = 30.0, iters: int = 500, encoder: str = "q", bank_samples: int = 256,
                 batch_size: int = 32, n_crop: int = 1, seed: int = 0):
        self._check_encoder(encoder)
        self._check_at_least_1(every=every, bank_samples=bank_samples, batch_size=batch_size, n_crop=n_crop)
        check_limits(bank_samples, 2, perplexity, iters)
        self.every, self.num_epochs, self.perplexity, self.iters = int(every), int(num_epochs), float(perplexity), int(iters)
        self.encoder, self.bank_samples, self.batch_size = encoder, int(bank_samples), int(batch_size)
        self.n_crop, self.seed = int(n_crop), int(seed)

    def build_loaders(self, T: int, size: int, device, seed: int = 0) -> tuple:
        """The kNN monitor's stand-in bank: split 'train' of ``SyntheticLabelledClips``."""
        return _knn.synthetic_loaders(self.bank_samples, 1, self.batch_size, self.NUM_CLASSES, self.n_crop, T, size, device, seed)[:1]

    def run(self, model: nn.Module, bank_loader: Iterable, out_prefix: Optional[str] = None, image_size: int = 512) -> dict:
        """{"kl", "purity", "n_bank", "bad_rows", "seconds"}; with ``out_prefix`` the map goes to out_prefix + ".npy" and ".png"."""
        self._refuse_capture()
        t0 = time.perf_counter()
        with _knn.frozen_encoder(model, self.encoder) as enc:
            g, y_g = _knn.extract_bank(enc, bank_loader, self.n_crop)
        with torch.no_grad():
            perp = min(self.perplexity, max(1.0, (g.shape[0] - 1) / 3.0))
            res = fit(g, perp, self.iters, exag_iters=min(250, self.iters // 2), seed=self.seed)
        ymap, lab = res.y.cpu().numpy(), y_g.cpu().numpy()
        if out_prefix is not None:
            np.save(out_prefix + ".npy", ymap)
            draw(ymap, lab, image_size).save(out_prefix + ".png")
        return {"kl": float(res.kl_trace[-1]), "purity": neighbour_purity(ymap, lab, 10), "n_bank": int(g.shape[0]),
                "bad_rows": res.info["rows_bad"], "seconds": time.perf_counter() - t0}

    def run_epoch(self, model, loaders: tuple, ctx: dict) -> dict:
        """The map goes to tsne_epoch{E}.npy / .png in the run directory."""
        return self.run(model, *loaders, os.path.join(ctx["run_dir"], f"tsne_epoch{ctx['epoch']}"))

    def scalars(self, result: dict) -> dict:
        return {"tsne_kl": result["kl"], "tsne_purity": result["purity"]}

    def log_line(self, result: dict, ctx: dict) -> str:
        r = result
        return (f"t-SNE [{ctx['epoch']}/{ctx['num_epochs']}]\tKL {r['kl']:.4f}\tpurity@10 {r['purity']:.4f}"
                f"\t(perplexity {self.perplexity:g}, {self.iters} iterations, bank {r['n_bank']}, {r['bad_rows']} bad, {r['seconds']:.1f} s)")


# ---- command line over saved retrieval features --------------------------------------------------------------------------
def map_features(feature_dir: str, fold: int, split: str = "train", perplexity: float = 30.0, iters: int = 1000, seed: int = 0,
                 max_rows: Optional[int] = None, init: str = "random", size: int = 1024, device=None) -> dict:
    """The t-SNE map of the train or test features ``rspnet_amd.retrieval`` saved (more than ``max_rows`` -- at most 16384 -- rows:
    a sub-sample drawn by a generator of this call's own).  Writes ``tsne_fold{F}.npy``, ``.png`` and ``.json``."""
    from .retrieval import load_features
    if split not in ("train", "test"):
        raise ValueError(f"tsne: split must be 'train' or 'test', got {split!r}")
    X_train, y_train, X_test, y_test = load_features(feature_dir, fold)
    X, y = (X_train, y_train) if split == "train" else (X_test, y_test)
    X, y = np.asarray(X), np.asarray(y)
    cap = MAX_ROWS if max_rows is None else min(int(max_rows), MAX_ROWS)
    if X.shape[0] > cap:
        pick = np.sort(np.random.default_rng(int(seed)).choice(X.shape[0], cap, replace=False))
        X, y = X[pick], y[pick]
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    res = fit(torch.as_tensor(X, dtype=torch.float32).to(torch.device(device)).contiguous(), perplexity, iters, seed=seed, init=init)
    ymap = res.y.cpu().numpy()
    out = {"split": split, "rows": int(X.shape[0]), "perplexity": float(perplexity), "iters": int(iters), "seed": int(seed), "init": init,
           "kl": float(res.kl_trace[-1]), "purity": neighbour_purity(ymap, y, 10), "info": res.info}
    base = os.path.join(feature_dir, f"tsne_fold{fold}")
    np.save(base + ".npy", ymap)
    draw(ymap, y, size).save(base + ".png")
    with open(base + ".json", "w") as fp:
        json.dump(out, fp)
    logger.info("t-SNE of {} {} rows: KL = {:.4f}, purity@10 = {:.4f} ({} invalid)".format(out["rows"], split, out["kl"], out["purity"],
                                                                                         res.info["rows_bad"]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="t-SNE map of a directory of saved retrieval features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--split", choices=("train", "test"), default="train")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-rows", type=int, default=None, help="sub-sample to at most this many rows (the limit is 16384)")
    ap.add_argument("--init", choices=("random", "pca"), default="random")
    ap.add_argument("--size", type=int, default=1024, help="side of the PNG in pixels")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return map_features(args.features, args.fold, args.split, args.perplexity, args.iters, args.seed, args.max_rows, args.init, args.size)


if __name__ == "__main__":
    main()
