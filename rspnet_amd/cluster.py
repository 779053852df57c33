"""Clustering evaluation: spherical k-means on frozen features, scored against the labels with NMI, ARI and purity -- the read of a
self-supervised representation that needs neither a labelled bank (kNN, retrieval) nor a trained head (the probe): do the classes form
modes of their own on the sphere?  The objective and the cluster sizes need no labels at all.  On the HIP backend ONE call,
rsp_kmeans_fit (csrc/cluster.hip), issues every iteration and stops on the device; rsp_contingency counts the cluster x label table;
the scores are formed from that table in numpy fp64 on the host.

The rule (include/rspnet_hip.h states it for the kernels; ``kmeans_reference`` restates it in numpy fp64):

    valid rows  the fp32 sum of squares of the row is finite and > 0.  An invalid row gets assign = -1, is counted in rows_bad and
                takes part in nothing
    assignment  the single neighbour of the cosine search (``rsp_cosine_topk`` with the centroids as the gallery, k = 1):
                s = (x_i . m_c) / (|x_i| |m_c|), a zero centroid has inverse norm 0, a centroid holding a NaN or an Inf is never
                returned, an exact tie goes to the lower cluster; a valid row without a returnable centroid gets -1 (``unassigned``)
    iteration   t = 0 .. max_iters - 1: assign; changed[t] = rows whose assignment differs from iteration t - 1 (t = 0: the valid rows);
                objective[t] = mean similarity of the assigned rows; t > 0 and changed[t] == 0: converged, iters_run = t + 1, stop.
                Otherwise cent[c] = sum of x_i / |x_i| over the rows of cluster c, unnormalised, stored in fp32; an empty cluster
                keeps its centroid.  The update also follows the last iteration of a fit that has not converged.
    traces      entries past iters_run: changed = -1, objective = NaN

Limits, enforced here with ValueError as the kernel enforces them with RSP_EINVAL: 1 <= N <= 262144, D even and 2 <= D <= 4096,
1 <= clusters <= 1024, 1 <= classes <= 1024, 1 <= max_iters <= 1000.

``ClusterMonitor`` is the pretext driver's opt-in hook (config key ``cluster_monitor``); ``python -m rspnet_amd.cluster --features DIR
--fold F`` clusters the features ``rspnet_amd.retrieval`` saved.  The monitor has run on one GPU only.
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

from . import _lib
from . import knn as _knn
from . import ops as _ops
from .framework.monitor import EpochMonitor
from .knn import _rows, _valid_rows_np, _valid_rows_torch

logger = logging.getLogger(__name__)
MAX_ROWS, MAX_CLUSTERS, MAX_CLASSES, MAX_D, MAX_ITERS = 262144, 1024, 1024, 4096, 1000

# of fit: tensors on x's device (changed / objective: max_iters entries), info: a dict on the host
KMeans = collections.namedtuple("KMeans", "cent assign counts changed objective info")
# of kmeans_reference: numpy; cents[t] (fp32) are the centroids iteration t assigned from, assigns[t] / sims[t] / gaps[t] its
# assignment, best similarity and best-to-second gap per row (fp64; NaN / inf on rows that are not assigned)
KMeansRef = collections.namedtuple("KMeansRef", "cent assign counts changed objective info cents assigns sims gaps")
INFO_KEYS = ("rows_valid", "rows_bad", "iters_run", "converged", "empty", "unassigned")


def check_limits(N, D, num_clusters, max_iters=1, num_classes=1):
    """ValueError for values rsp_kmeans_fit / rsp_kmeans_assign / rsp_contingency would reject."""
    if not 1 <= int(N) <= MAX_ROWS:
        raise ValueError(f"cluster: N must be in [1, {MAX_ROWS}], got {N}")
    if not (2 <= int(D) <= MAX_D and int(D) % 2 == 0):
        raise ValueError(f"cluster: D must be even and in [2, {MAX_D}], got {D}")
    if not 1 <= int(num_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"cluster: num_clusters must be in [1, {MAX_CLUSTERS}], got {num_clusters}")
    if not 1 <= int(max_iters) <= MAX_ITERS:
        raise ValueError(f"cluster: max_iters must be in [1, {MAX_ITERS}], got {max_iters}")
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"cluster: num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")


# ---- the definition in numpy fp64 ----------------------------------------------------------------------------------------
def reference_similarities(x, cent) -> np.ndarray:
    """(N, C) fp64 similarities of the rule: -inf in the column of a centroid that holds a NaN or an Inf (never returned), NaN in
    the row of an invalid row."""
    x32, c32 = np.asarray(x, dtype=np.float32), np.asarray(cent, dtype=np.float32)
    ok = _valid_rows_np(x32)
    sim = np.full((x32.shape[0], c32.shape[0]), np.nan)
    cfinite = np.isfinite(c32).all(axis=1)
    c64 = np.where(cfinite[:, None], c32, 0).astype(np.float64)
    cn = np.linalg.norm(c64, axis=1)
    with np.errstate(all="ignore"):
        css = (c32 * c32).sum(axis=1, dtype=np.float32)      # (a centroid whose fp32 sum of squares overflows has inverse norm 0)
        cinv = np.where((cn > 0) & np.isfinite(css), 1.0 / np.where(cn > 0, cn, 1.0), 0.0)
    a = x32[ok].astype(np.float64)
    s = (a @ c64.T) * (1.0 / np.linalg.norm(a, axis=1, keepdims=True)) * cinv[None, :]
    s[:, ~cfinite] = -np.inf
    sim[ok] = s
    return sim


def _assign_np(sim: np.ndarray):
    """(assign, best, gap) per row of an (N, C) similarity matrix: first maximum (the lower cluster on a tie), -1 where the row is
    NaN or holds nothing above -inf."""
    N, C = sim.shape
    rows_ok = ~np.isnan(sim).any(axis=1)
    s = np.where(rows_ok[:, None], sim, -np.inf)
    a = s.argmax(axis=1)
    best = s[np.arange(N), a]
    got = rows_ok & (best > -np.inf)
    rest = s.copy()
    rest[np.arange(N), a] = -np.inf
    second = rest.max(axis=1) if C > 1 else np.full(N, -np.inf)
    with np.errstate(invalid="ignore"):
        gap = np.where(got, best - second, np.inf)
    return np.where(got, a, -1).astype(np.int64), np.where(got, best, np.nan), gap


def update_reference(x, assign, cent) -> np.ndarray:
    """The update of the rule in fp64 (not rounded): row c = the sum of x_i / |x_i| over assign == c; an empty cluster keeps cent[c]."""
    x32 = np.asarray(x, dtype=np.float32)
    out = np.array(cent, dtype=np.float64)
    for c in np.unique(assign[assign >= 0]):
        a = x32[assign == c].astype(np.float64)
        out[c] = (a / np.linalg.norm(a, axis=1, keepdims=True)).sum(axis=0)
    return out


def kmeans_reference(x, init, max_iters: int) -> KMeansRef:
    """The rule of the module docstring in numpy fp64, with the fp32 storage of the centroids between iterations (validity is decided
    on the fp32 sum of squares, as the kernel decides it)."""
    x32 = np.asarray(x, dtype=np.float32)
    cent = np.array(init, dtype=np.float32)
    N, C = x32.shape[0], cent.shape[0]
    ok = _valid_rows_np(x32)
    changed = np.full(int(max_iters), -1, dtype=np.int64)
    objective = np.full(int(max_iters), np.nan)
    cents, assigns, sims, gaps = [], [], [], []
    prev, converged, iters_run = None, 0, int(max_iters)
    for t in range(int(max_iters)):
        cents.append(cent.copy())
        a, best, gap = _assign_np(reference_similarities(x32, cent))
        assigns.append(a)
        sims.append(best)
        gaps.append(gap)
        changed[t] = int(ok.sum()) if prev is None else int((a != prev)[ok].sum())
        objective[t] = float(best[a >= 0].mean()) if (a >= 0).any() else 0.0
        prev = a
        if t > 0 and changed[t] == 0:
            converged, iters_run = 1, t + 1
            break
        cent = update_reference(x32, a, cent).astype(np.float32)
    counts = np.bincount(prev[prev >= 0], minlength=C).astype(np.int64)
    info = {"rows_valid": int(ok.sum()), "rows_bad": int(N - ok.sum()), "iters_run": iters_run, "converged": converged,
            "empty": int((counts == 0).sum()), "unassigned": int((ok & (prev < 0)).sum())}
    return KMeansRef(cent, prev, counts, changed, objective, info, cents, assigns, sims, gaps)


# ---- the same rule from torch ops ----------------------------------------------------------------------------------------
def _assign_torch(x: Tensor, cent: Tensor):
    """(assign int32, sim fp32) of the rule from torch ops (this one stores the N x C matrix)."""
    ok = _valid_rows_torch(x)
    xn = x.norm(dim=1, keepdim=True)
    cs = (cent * cent).sum(dim=1)
    cinv = torch.where(torch.isfinite(cs) & (cs > 0), 1.0 / cent.norm(dim=1), torch.zeros_like(cs))
    xs = torch.where(ok[:, None], x, torch.zeros_like(x))                            # selected away, not multiplied
    sim = (xs @ cent.t()) * torch.where(ok[:, None], 1.0 / xn, torch.zeros_like(xn)) * cinv[None, :]
    sim = torch.where(sim == sim, sim, torch.full_like(sim, -math.inf))              # a NaN similarity is never returned
    best, a = sim.max(dim=1)                                                        # the first maximum: the lower cluster
    got = ok & (best > -math.inf)
    return torch.where(got, a, torch.full_like(a, -1)).to(torch.int32), torch.where(got, best, torch.full_like(best, math.nan))


def _kmeans_torch(x: Tensor, cent: Tensor, max_iters: int):
    """The rule from torch ops on whatever device the tensors are on; cent changes in place.  The stop is read back every iteration:
    this is the fallback.  Returns (assign, counts, changed, objective, info dict)."""
    N, C = x.shape[0], cent.shape[0]
    ok = _valid_rows_torch(x)
    m = int(ok.sum())
    xh = torch.where(ok[:, None], x / x.norm(dim=1, keepdim=True), torch.zeros_like(x))
    changed = torch.full((max_iters,), -1, dtype=torch.int32, device=x.device)
    objective = torch.full((max_iters,), math.nan, dtype=torch.float64, device=x.device)
    prev, converged, iters_run = None, 0, max_iters
    counts = torch.zeros(C, dtype=torch.int32, device=x.device)
    for t in range(max_iters):
        a, sim = _assign_torch(x, cent)
        got = a >= 0
        changed[t] = m if prev is None else int(((a != prev) & ok).sum())
        objective[t] = sim[got].to(torch.float64).mean() if bool(got.any()) else 0.0
        prev = a
        if t > 0 and int(changed[t]) == 0:
            converged, iters_run = 1, t + 1
            break
        idx = a[got].to(torch.int64)
        counts = torch.bincount(idx, minlength=C).to(torch.int32)
        sums = torch.zeros_like(cent).index_add_(0, idx, xh[got])
        cent.copy_(torch.where((counts > 0)[:, None], sums, cent))
    info = {"rows_valid": m, "rows_bad": N - m, "iters_run": iters_run, "converged": converged, "empty": int((counts == 0).sum()),
            "unassigned": int((ok & (prev < 0)).sum())}
    return prev, counts, changed, objective, info


def _contingency_torch(assign: Tensor, y: Tensor, C: int, L: int):
    good = (assign >= 0) & (assign < C) & (y >= 0) & (y < L)
    flat = assign[good].to(torch.int64) * L + y[good]
    table = torch.bincount(flat, minlength=C * L).view(C, L).to(torch.int64)
    return table, (~good).sum().to(torch.int64).reshape(1)


# ---- the public calls ----------------------------------------------------------------------------------------------------
def read_info(info: Tensor) -> dict:
    """The 32-byte rsp_kmeans_info of HipOps.kmeans_fit as a dict (one small copy to the host)."""
    rec = _lib.KmeansInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return {k: int(getattr(rec, k)) for k in INFO_KEYS}


def fit_raw(x: Tensor, cent: Tensor, max_iters: int) -> KMeans:
    """``max_iters`` iterations from the centroids ``cent``, which change in place: one rsp_kmeans_fit call when the active op backend
    has ``kmeans_fit``, the same rule from torch ops otherwise."""
    check_limits(x.shape[0], x.shape[1], cent.shape[0], max_iters)
    be = _ops.backend()
    if hasattr(be, "kmeans_fit"):
        r = be.kmeans_fit(x, cent, int(max_iters))
        return KMeans(cent, r.assign, r.counts, r.changed, r.objective, read_info(r.info))
    a, counts, changed, objective, info = _kmeans_torch(x, cent, int(max_iters))
    return KMeans(cent, a, counts, changed, objective, info)


def fit(x: Tensor, num_clusters: int, max_iters: int = 50, seed: int = 0, init: Optional[Tensor] = None, restarts: int = 1) -> KMeans:
    """Spherical k-means on the rows of x (N, D).  The initial centroids are ``init`` (num_clusters, D), or ``num_clusters`` distinct
    valid rows of x drawn by a generator of this call's own seeded with ``seed`` (no global generator is drawn from); ValueError with
    fewer valid rows than clusters.  restarts > 1 (without ``init``): that many draws from the same generator, the fit with the largest
    final objective is kept.  Returns KMeans(cent, assign, counts, changed, objective, info)."""
    N, D = x.shape
    C = int(num_clusters)
    check_limits(N, D, C, max_iters)
    if int(restarts) < 1:
        raise ValueError(f"cluster: restarts must be at least 1, got {restarts}")
    x = _rows(x)
    if init is not None:
        if tuple(init.shape) != (C, D):
            raise ValueError(f"cluster: init must be ({C}, {D}), got {tuple(init.shape)}")
        return fit_raw(x, init.to(x.device, torch.float32).clone().contiguous(), max_iters)
    gen = torch.Generator().manual_seed(int(seed))
    ok = _valid_rows_torch(x)
    best = None
    for _ in range(int(restarts)):
        perm = torch.randperm(N, generator=gen).to(x.device)
        picked = perm[ok.index_select(0, perm)][:C]      # the first num_clusters valid rows of a random order: distinct
        if picked.numel() < C:
            raise ValueError(f"cluster: {C} clusters need at least as many valid rows")
        res = fit_raw(x, x.index_select(0, picked).contiguous(), max_iters)
        if int(restarts) == 1:
            return res
        score = float(res.objective[res.info["iters_run"] - 1])
        if best is None or score > best[0]:
            best = (score, res)
    return best[1]


def assign(fitted, x: Tensor):
    """(assign int32 (N,), sim fp32 (N,)) of new rows against the fitted centroids (a KMeans, or the centroid matrix itself)."""
    cent = fitted.cent if hasattr(fitted, "cent") else fitted
    x = _rows(x)
    check_limits(x.shape[0], x.shape[1], cent.shape[0])
    be = _ops.backend()
    if hasattr(be, "kmeans_assign"):
        return be.kmeans_assign(x, cent.contiguous())
    return _assign_torch(x, cent)


def contingency(assign_: Tensor, y: Tensor, num_clusters: int, num_classes: int):
    """(table int64 (num_clusters, num_classes), dropped int64 (1,)) on the device: table[c][l] = the rows with assign == c and
    y == l; a row with assign < 0 or a label outside [0, num_classes) is counted in dropped."""
    check_limits(assign_.numel(), 2, num_clusters, 1, num_classes)
    a = assign_.to(torch.int32).reshape(-1).contiguous()
    y = y.to(torch.int64).reshape(-1).contiguous()
    be = _ops.backend()
    if hasattr(be, "contingency"):
        return be.contingency(a, y, int(num_clusters), int(num_classes))
    return _contingency_torch(a, y, int(num_clusters), int(num_classes))


def _entropy(counts: np.ndarray) -> float:
    p = counts[counts > 0].astype(np.float64)
    if p.size == 0:
        return 0.0
    p = p / p.sum()
    return float(-(p * np.log(p)).sum())


def scores(table) -> dict:
    """From the cluster x label table (rows: clusters), in numpy fp64 on the host: {"nmi" (arithmetic-mean normalisation), "ari",
    "purity", "size_entropy" (entropy of the cluster sizes over log(#clusters); 0 with one cluster), "n"}, and "hungarian_acc" --
    the accuracy under the best one-to-one matching of clusters to labels -- where scipy.optimize.linear_sum_assignment imports."""
    t = np.asarray(table.cpu() if isinstance(table, Tensor) else table).astype(np.int64)
    n = int(t.sum())
    a, b = t.sum(axis=1), t.sum(axis=0)
    out = {"n": n}
    if n == 0:
        out.update(nmi=0.0, ari=0.0, purity=0.0, size_entropy=0.0)
        return out
    hu, hv = _entropy(a), _entropy(b)
    nz = t > 0
    pij = t[nz].astype(np.float64) / n
    outer = (a[:, None].astype(np.float64) * b[None, :].astype(np.float64))[nz] / (float(n) * float(n))
    mi = max(float((pij * (np.log(pij) - np.log(outer))).sum()), 0.0)
    if (a > 0).sum() == 1 and (b > 0).sum() == 1:
        nmi = 1.0                                   # both partitions trivial: identical
    else:
        nmi = mi / max(0.5 * (hu + hv), np.finfo(np.float64).eps)
    comb = lambda v: int((v.astype(object) * (v.astype(object) - 1) // 2).sum())      # exact integers
    sij, sa, sb, tot = comb(t.reshape(-1)), comb(a), comb(b), n * (n - 1) // 2
    # pair counts (tp = sij, fp = sa - sij, fn = sb - sij, tn = the rest): 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn))
    tp, fp, fn = sij, sa - sij, sb - sij
    tn = tot - tp - fp - fn
    ari = 1.0 if (fp == 0 and fn == 0) else 2.0 * (tp * tn - fn * fp) / float((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    C = t.shape[0]
    out.update(nmi=float(nmi), ari=float(ari), purity=float(t.max(axis=1).sum()) / n,
               size_entropy=_entropy(a) / math.log(C) if C > 1 else 0.0)
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return out
    r, c = linear_sum_assignment(-t)
    out["hungarian_acc"] = float(t[r, c].sum()) / n
    return out


def evaluate(x: Tensor, y: Tensor, num_clusters: int, num_classes: Optional[int] = None, max_iters: int = 50, seed: int = 0,
             init: Optional[Tensor] = None, restarts: int = 1) -> dict:
    """fit, contingency and scores chained: the scores, plus "objective" (of the last iteration run), "iters", "converged", "empty",
    "bad_rows", "unassigned", "dropped" and "fit" (the KMeans).  What comes to the host: the C x L table, the traces and info."""
    if num_classes is None:
        num_classes = int(y.max()) + 1
    check_limits(x.shape[0], x.shape[1], num_clusters, max_iters, num_classes)
    res = fit(x, num_clusters, max_iters, seed, init, restarts)
    table, dropped = contingency(res.assign, y.to(res.assign.device), num_clusters, num_classes)
    out = scores(table)
    info = res.info
    out.update(objective=float(res.objective[info["iters_run"] - 1]), iters=info["iters_run"], converged=info["converged"],
               empty=info["empty"], bad_rows=info["rows_bad"], unassigned=info["unassigned"], dropped=int(dropped), fit=res)
    return out


# ---- the pretext driver's hook -------------------------------------------------------------------------------------------
class ClusterMonitor(EpochMonitor):
    """Every ``every``-th epoch (and on the last one): k-means on the backbone features of a labelled bank from one encoder of the
    pretext model (``knn.extract``), scored against the bank's labels.  ``run`` leaves the model as it found it -- state_dict() bit for
    bit, every module's ``training`` flag --, draws from no global random generator and refuses to run inside a graph capture.  Has
    run on one GPU only.  Config, e.g. {"every": 10, "num_clusters": 101, "num_classes": 101}."""

    KEY = "cluster_monitor"
    KEYS = ("every", "num_clusters", "num_classes", "encoder", "bank_samples", "batch_size", "n_crop", "max_iters", "seed", "restarts")

    def __init__(self, every: int, num_epochs: int, num_clusters: int = 101, num_classes: int = 101, encoder: str = "q",
                 bank_samples: int = 256, batch_size: int = 32, n_crop: int = 1, max_iters: int = 50, seed: int = 0, restarts: int = 1):
        self._check_encoder(encoder)
        self._check_at_least_1(every=every, bank_samples=bank_samples, batch_size=batch_size, n_crop=n_crop, restarts=restarts)
        check_limits(bank_samples, 2, num_clusters, max_iters, num_classes)
        if int(num_clusters) > int(bank_samples):
            raise ValueError(f"cluster_monitor: {num_clusters} clusters need at least as many bank samples, got {bank_samples}")
        self.every, self.num_epochs = int(every), int(num_epochs)
        self.num_clusters, self.num_classes, self.encoder = int(num_clusters), int(num_classes), encoder
        self.bank_samples, self.batch_size, self.n_crop = int(bank_samples), int(batch_size), int(n_crop)
        self.max_iters, self.seed, self.restarts = int(max_iters), int(seed), int(restarts)

    def build_loaders(self, T: int, size: int, device, seed: int = 0) -> tuple:
        """The kNN monitor's stand-in bank: split 'train' of ``SyntheticLabelledClips``."""
        return _knn.synthetic_loaders(self.bank_samples, 1, self.batch_size, self.num_classes, self.n_crop, T, size, device, seed)[:1]

    def run(self, model: nn.Module, bank_loader: Iterable) -> dict:
        """{"nmi", "ari", "purity", "objective", "iters", "empty", "n_bank", "bad_rows", "seconds"}."""
        self._refuse_capture()
        t0 = time.perf_counter()
        with _knn.frozen_encoder(model, self.encoder) as enc:
            g, y_g = _knn.extract_bank(enc, bank_loader, self.n_crop)
        with torch.no_grad():
            res = evaluate(g, y_g, self.num_clusters, self.num_classes, self.max_iters, self.seed, restarts=self.restarts)
        return {"nmi": res["nmi"], "ari": res["ari"], "purity": res["purity"], "objective": res["objective"], "iters": res["iters"],
                "empty": res["empty"], "n_bank": int(g.shape[0]), "bad_rows": res["bad_rows"], "seconds": time.perf_counter() - t0}

    def scalars(self, result: dict) -> dict:
        return {f"cluster_{k}": result[k] for k in ("nmi", "ari", "purity", "objective", "iters", "empty")}

    def log_line(self, result: dict, ctx: dict) -> str:
        r = result
        return (f"Cluster [{ctx['epoch']}/{ctx['num_epochs']}]\tNMI {r['nmi']:.4f}\tARI {r['ari']:.4f}\tpurity {r['purity']:.4f}"
                f"\tobjective {r['objective']:.4f}\t({self.num_clusters} clusters, {r['iters']} iterations, {r['empty']} empty, "
                f"bank {r['n_bank']}, {r['bad_rows']} bad, {r['seconds']:.1f} s)")


# ---- command line over saved retrieval features --------------------------------------------------------------------------
def cluster_features(feature_dir: str, fold: int, split: str = "train", clusters: Optional[int] = None, iters: int = 50, seed: int = 0,
                     restarts: int = 1, device=None) -> dict:
    """k-means over the train or test features ``rspnet_amd.retrieval`` saved, scored against their labels; the default number of
    clusters is the largest label + 1.  Logs one line and writes ``cluster_fold{F}.json``."""
    from .retrieval import load_features
    if split not in ("train", "test"):
        raise ValueError(f"cluster: split must be 'train' or 'test', got {split!r}")
    X_train, y_train, X_test, y_test = load_features(feature_dir, fold)
    X, y = (X_train, y_train) if split == "train" else (X_test, y_test)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(device)
    num_classes = int(y.max()) + 1
    C = num_classes if clusters is None else int(clusters)
    res = evaluate(torch.as_tensor(X, dtype=torch.float32).to(dev).contiguous(), torch.as_tensor(y).to(dev), C, num_classes, iters, seed,
                   restarts=restarts)
    logger.info("k-means C={} on {} {} rows: NMI = {:.4f}, ARI = {:.4f}, purity = {:.4f}, objective {:.4f} ({} iterations, {} empty)".format(
        C, res["n"], split, res["nmi"], res["ari"], res["purity"], res["objective"], res["iters"], res["empty"]))
    out = {k: v for k, v in res.items() if k != "fit"}
    out.update(split=split, clusters=C, num_classes=num_classes, max_iters=int(iters), seed=int(seed), restarts=int(restarts))
    with open(os.path.join(feature_dir, f"cluster_fold{fold}.json"), "w") as fp:
        json.dump(out, fp)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="k-means clustering evaluation over a directory of saved retrieval features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--split", choices=("train", "test"), default="train")
    ap.add_argument("--clusters", type=int, default=None, help="number of clusters (default: the largest label + 1)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restarts", type=int, default=1)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return cluster_features(args.features, args.fold, args.split, args.clusters, args.iters, args.seed, args.restarts)


if __name__ == "__main__":
    main()
