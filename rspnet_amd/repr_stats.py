"""Label-free representation statistics: whether a set of embeddings spreads over the sphere or collapses, without a single label.
The project's own (the reference has no such monitor); the definitions are the published ones.

    uniformity       log mean_{i<j} exp(-t |xi - xj|^2) over the unit rows (Wang & Isola 2020); |xi - xj|^2 = 2 - 2 s, so the term is
                     exp(2 t (s - 1)).  More negative is more uniform; 0 is collapse.
    mean_cos(2)      mean (squared) pairwise cosine s over i < j
    effective_rank   RankMe (Garrido et al. 2023): exp of the entropy of the normalised singular values of the unit-row matrix, which
                     are the square roots of the eigenvalues of its D x D Gram matrix
    dim_std_*        standard deviation of each coordinate of the unit rows times sqrt(D): 1 when isotropic, 0 when collapsed

On the HIP backend the pair sums, the Gram matrix and the column sums are ONE call (rsp_repr_stats, csrc/repr_stats.hip): the N x N
similarity matrix is never stored.

The rule (include/rspnet_hip.h states it for the kernel; ``repr_reference`` restates it in numpy fp64):

    validity   ss_i = the fp32 sum of squares of row i; the row is valid iff ss_i is finite and > 0 (a zero row, a row holding a NaN or
               an Inf: invalid).  An invalid row takes part in nothing; M = the number of valid rows.
    s_ij       (x_i . x_j) * inv_i * inv_j, inv_i = 1 / sqrtf(ss_i) in fp32
    pair sums  over valid i < j, each pair once: pair_exp = sum exp(c (s - 1)) with c = 2 t, pair_cos = sum s, pair_cos2 = sum s^2
    gram       gram[a][b] = sum over valid i of xh_ia xh_ib, colsum[a] = sum over valid i of xh_ia, xh = x * inv formed in fp32

Limits of the kernel, enforced here as well: t finite and in (0, 32] (c = 2 t in (0, 64]).

``ReprMonitor`` is the pretext driver's opt-in hook (config key ``repr_monitor``): the statistics of the MoCo queue, the last K key
embeddings, which are on the device anyway.  ``python -m rspnet_amd.repr_stats --features DIR --fold F`` computes them over the
features ``rspnet_amd.retrieval`` saved.
"""
from __future__ import annotations

import argparse
import json
import logging
import math
import os
import time
import numpy as np
import torch
from torch import Tensor, nn

from . import _lib
from . import ops as _ops
from .framework.monitor import EpochMonitor

logger = logging.getLogger(__name__)
MAX_T = 32.0


def check_limits(t):
    """ValueError for a temperature rsp_repr_stats would reject."""
    if not (math.isfinite(float(t)) and 0.0 < float(t) <= MAX_T):
        raise ValueError(f"repr_stats: t must be finite and in (0, {MAX_T:g}], got {t}")


# ---- the definition in numpy fp64 ----------------------------------------------------------------------------------------
def _row_sumsq_fp32(x: np.ndarray) -> np.ndarray:
    """The fp32 sum of squares of every row in the kernel's order: lane l of 64 takes the column pairs 2 l, 2 l + 128, ... by fmaf (x,
    then y), then the xor butterfly 32, 16, ... 1.  (fmaf as the fp64 product and sum rounded once to fp32: the product is exact.)"""
    N, D = x.shape
    cols = 128 * ((D + 127) // 128)
    xp = np.zeros((N, cols), dtype=np.float64)
    xp[:, :D] = x
    lanes = np.zeros((N, 64), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(0, cols, 128):
            blk = xp[:, c:c + 128].reshape(N, 64, 2)
            for j in range(2):
                lanes = (blk[:, :, j] * blk[:, :, j] + lanes.astype(np.float64)).astype(np.float32)
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def repr_reference(x, t: float = 2.0) -> dict:
    """The rule of the module docstring in numpy fp64, validity and the inverse norms in fp32 as stated.  Returns {"pair_exp",
    "pair_cos", "pair_cos2", "rows_valid", "rows_bad", "gram" (D, D), "colsum" (D,)}.  Stores the M x M matrix."""
    check_limits(t)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    N, D = x.shape
    ss = _row_sumsq_fp32(x)
    valid = np.isfinite(ss) & (ss > 0)
    xv = x[valid]
    inv = (np.float32(1.0) / np.sqrt(ss[valid], dtype=np.float32)).astype(np.float32)
    M = int(valid.sum())
    x64, inv64 = xv.astype(np.float64), inv.astype(np.float64)
    s = (x64 @ x64.T) * inv64[:, None] * inv64[None, :]
    upper = s[np.triu_indices(M, k=1)]
    xh = (xv * inv[:, None]).astype(np.float32).astype(np.float64)
    return {"pair_exp": float(np.exp(2.0 * float(t) * (upper - 1.0)).sum()), "pair_cos": float(upper.sum()),
            "pair_cos2": float((upper * upper).sum()), "rows_valid": M, "rows_bad": N - M, "gram": xh.T @ xh, "colsum": xh.sum(axis=0)}


# ---- the statistics ------------------------------------------------------------------------------------------------------
def _raw_torch(x: Tensor, t: float, block: int = 2048) -> dict:
    """The same sums from torch ops on whatever device x is on (this one stores block x M pieces of the similarity matrix)."""
    x = x.to(torch.float32)
    ss = (x * x).sum(dim=1)
    valid = torch.isfinite(ss) & (ss > 0)
    xv = x[valid]
    inv = 1.0 / ss[valid].sqrt()
    M = int(xv.shape[0])
    col = torch.arange(M, device=x.device)
    c = np.float32(2.0 * float(t))
    pe = pc = pc2 = 0.0
    for r0 in range(0, M, block):
        s = (xv[r0:r0 + block] @ xv.t()) * inv[r0:r0 + block, None] * inv[None, :]
        keep = col[None, :] > col[r0:r0 + block, None]
        sk = s[keep].double()
        pe += float(torch.exp(c * (s[keep] - 1.0)).double().sum())
        pc += float(sk.sum())
        pc2 += float((sk * sk).sum())
    xh = (xv * inv[:, None]).double()
    return {"pair_exp": pe, "pair_cos": pc, "pair_cos2": pc2, "rows_valid": M, "rows_bad": int(x.shape[0]) - M,
            "gram": (xh.t() @ xh).cpu().numpy(), "colsum": xh.sum(dim=0).cpu().numpy()}


def raw_stats(x: Tensor, t: float = 2.0) -> dict:
    """{"pair_exp", "pair_cos", "pair_cos2", "rows_valid", "rows_bad", "gram", "colsum"} of the rows of x, on the host: one
    rsp_repr_stats call and one read of its three outputs when the active op backend has ``repr_stats``; torch ops otherwise."""
    check_limits(t)
    be = _ops.backend()
    if not hasattr(be, "repr_stats"):
        return _raw_torch(x, t)
    res = be.repr_stats(x.to(torch.float32), float(t))
    sums = _lib.ReprSums.from_buffer_copy(res.sums.cpu().numpy().tobytes())
    return {"pair_exp": sums.pair_exp, "pair_cos": sums.pair_cos, "pair_cos2": sums.pair_cos2, "rows_valid": int(sums.rows_valid),
            "rows_bad": int(sums.rows_bad), "gram": res.gram.cpu().numpy(), "colsum": res.colsum.cpu().numpy()}


def summarize(raw: dict) -> dict:
    """The published statistics from the raw sums (of ``raw_stats`` or ``repr_reference``): fp64 on the host."""
    M, gram, colsum = int(raw["rows_valid"]), np.asarray(raw["gram"], dtype=np.float64), np.asarray(raw["colsum"], dtype=np.float64)
    D = gram.shape[0]
    nan = float("nan")
    pairs = M * (M - 1) / 2.0
    out = {"uniformity": (math.log(raw["pair_exp"] / pairs) if raw["pair_exp"] > 0 else -math.inf) if M >= 2 else nan,
           "mean_cos": raw["pair_cos"] / pairs if M >= 2 else nan, "mean_cos2": raw["pair_cos2"] / pairs if M >= 2 else nan}
    sigma = np.sqrt(np.maximum(np.linalg.eigvalsh(gram), 0.0))
    if M >= 1 and sigma.sum() > 0:
        p = sigma / sigma.sum() + 1e-7
        out["effective_rank"] = float(np.exp(-(p * np.log(p)).sum()))
        std = np.sqrt(np.maximum(np.diag(gram) / M - (colsum / M) ** 2, 0.0)) * math.sqrt(D)
        out["dim_std_min"], out["dim_std_mean"] = float(std.min()), float(std.mean())
    else:
        out["effective_rank"] = out["dim_std_min"] = out["dim_std_mean"] = nan
    out["rows"], out["bad_rows"] = M, int(raw["rows_bad"])
    return out


def repr_stats(x: Tensor, t: float = 2.0) -> dict:
    """{"uniformity", "mean_cos", "mean_cos2", "effective_rank", "dim_std_min", "dim_std_mean", "rows" (the valid ones), "bad_rows"}
    of the rows of x (N, D).  uniformity and the two means are NaN with fewer than two valid rows."""
    return summarize(raw_stats(x, t))


# ---- the pretext driver's hook -------------------------------------------------------------------------------------------
class ReprMonitor(EpochMonitor):
    """Every ``every``-th epoch (and on the last one): ``repr_stats`` of the pretext model's queue, the last K key embeddings as K x dim
    rows.  ``run`` reads the queue and nothing else: the model stays as it was bit for bit, no generator is drawn from, and it
    refuses to run inside a graph capture.  Config, e.g. {"every": 1, "t": 2.0}; no labels, no loaders."""

    KEY = "repr_monitor"
    KEYS = ("every", "t")

    def __init__(self, every: int, num_epochs: int, t: float = 2.0):
        check_limits(t)
        self._check_at_least_1(every=every)
        self.every, self.num_epochs, self.t = int(every), int(num_epochs), float(t)

    def run(self, model: nn.Module) -> dict:
        """``repr_stats`` of the queue plus "seconds".  ``model``: the pretext model (or its wrapper with ``.module``)."""
        self._refuse_capture()
        t0 = time.perf_counter()
        net = getattr(model, "module", model)
        with torch.no_grad():
            out = repr_stats(net.queue.t().contiguous(), self.t)
        out["seconds"] = time.perf_counter() - t0
        return out

    def run_epoch(self, model, loaders: tuple, ctx: dict) -> dict:
        """The statistics of the queue -- and, as "bank", of the bank features when the kNN monitor has just left them in ctx."""
        r = self.run(model)
        r["dim"] = getattr(model, "module", model).queue.shape[0]
        bank = ctx.pop("bank_features", None)
        if bank is not None:
            r["bank"] = dict(repr_stats(bank, self.t), dim=bank.shape[1])
        return r

    def scalars(self, result: dict) -> dict:
        rec = {f"repr/{k}": result[k] for k in ("uniformity", "mean_cos", "effective_rank", "dim_std_min", "bad_rows")}
        if "bank" in result:
            rec.update({f"repr/bank_{k}": result["bank"][k] for k in ("uniformity", "effective_rank", "dim_std_min")})
        return rec

    def log_line(self, result: dict, ctx: dict) -> str:
        r = result
        line = (f"Repr [{ctx['epoch']}/{ctx['num_epochs']}]\tuniformity {r['uniformity']:.4f}\teff.rank "
                f"{r['effective_rank']:.1f}/{r['dim']}\tmean cos {r['mean_cos']:.4f}\tdim std min "
                f"{r['dim_std_min']:.3f}\t(t={self.t}, {r['rows']} rows, {r['bad_rows']} bad, {r['seconds']:.2f} s)")
        if "bank" in r:
            b = r["bank"]
            line += f"\tbank: uniformity {b['uniformity']:.4f}\teff.rank {b['effective_rank']:.1f}/{b['dim']}"
        return line


# ---- command line over saved retrieval features --------------------------------------------------------------------------
def features_stats(feature_dir: str, fold: int, split: str = "train", t: float = 2.0, max_rows: int = 0, device=None) -> dict:
    """The statistics of the ``split`` features ``rspnet_amd.retrieval`` saved (float64 on disk, cast to fp32); ``max_rows`` N > 0 keeps
    every ceil(n / N)-th row.  Logs one line and writes ``repr_fold{F}.json``."""
    from .retrieval import load_features
    X_train, _, X_test, _ = load_features(feature_dir, fold)
    X = np.asarray(X_train if split == "train" else X_test)
    if max_rows and X.shape[0] > max_rows:
        X = X[::-(-X.shape[0] // int(max_rows))]
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    out = repr_stats(torch.as_tensor(X, dtype=torch.float32).to(torch.device(device)).contiguous(), t)
    out["t"] = float(t)
    logger.info("Repr {} fold {} t={}: uniformity {:.4f}, mean cos {:.4f}, eff.rank {:.1f}/{}, dim std min {:.3f} mean {:.3f}, "
                "{} rows ({} bad)".format(split, fold, t, out["uniformity"], out["mean_cos"], out["effective_rank"], X.shape[1],
                                          out["dim_std_min"], out["dim_std_mean"], out["rows"], out["bad_rows"]))
    with open(os.path.join(feature_dir, f"repr_fold{fold}.json"), "w") as fp:
        json.dump(out, fp)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="label-free representation statistics over a directory of saved retrieval features")
    ap.add_argument("--features", required=True, help="directory with {train,test}_fold{F}_{feats,labels}.npy")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--split", choices=("train", "test"), default="train")
    ap.add_argument("--t", type=float, default=2.0)
    ap.add_argument("--max-rows", type=int, default=0, help="keep every ceil(n / N)-th row (0: all)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return features_stats(args.features, args.fold, args.split, args.t, args.max_rows)


if __name__ == "__main__":
    main()
