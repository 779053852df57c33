#!/usr/bin/env python
"""Time of the clustering fit on one MI355X: rsp_kmeans_fit (one call: all iterations issued, stopped on the device) at the UCF-101
split-1 train size (9 537 x 512 -> 101 clusters) and at the MoCo queue's (16 384 x 128 -> 256), 20 iterations each; alongside, on the
same inputs and in the same process, the same Lloyd iteration composed from torch ops (matmul, max, index_add_: the library GEMM, float
atomics in the update, no stop -- it always runs all 20 iterations and reads nothing back; a measurement baseline, not a product
path).  Device events around one call each, every shape and every body warmed first, the two bodies interleaved repeat by repeat so
that they see the same state of the machine; median (min - max) ms per call, and next to it the host's issue time: the host clock
around the same call, before anything is waited for.

    python tools/cluster_bench.py [--repeats 21] [--out profiles/cluster_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import cluster, ops

SHAPES = [(9537, 512, 101), (16384, 128, 256)]      # N, D, clusters
ITERS = 20


def timed(fn):
    """(device ms between two events around fn, host ms until fn returned)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host


def lloyd_torch(x, init, iters):
    """The same iteration from torch ops, every iteration run, nothing read back: (cent, assign, objective of the last iteration)."""
    xh = x / x.norm(dim=1, keepdim=True)
    cent = init.clone()
    C = cent.shape[0]
    ones = torch.ones(x.shape[0], device=x.device)
    for _ in range(iters):
        sim = xh @ (cent / cent.norm(dim=1, keepdim=True)).t()
        best, a = sim.max(dim=1)
        sums = torch.zeros_like(cent).index_add_(0, a, xh)
        counts = torch.zeros(C, device=x.device).index_add_(0, a, ones)
        cent = torch.where((counts > 0)[:, None], sums, cent)
    return cent, a, best.mean()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats: a median of at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    be = ops.backend()
    lines = [f"cluster_bench: {torch.cuda.get_device_name(0)}, {ITERS} iterations per call, {args.repeats} interleaved repeats after "
             f"{args.warmup} warm-up calls, ms per call: device median (min - max) | host issue median"]
    for N, D, C in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        mu = torch.randn(C, D, device=dev, generator=gen)
        y = torch.randint(0, C, (N,), device=dev, generator=gen)
        x = 0.15 * mu[y] + torch.randn(N, D, device=dev, generator=gen)
        init = x[torch.randperm(N, generator=torch.Generator().manual_seed(2))[:C].to(dev)].contiguous()
        cent = init.clone()
        out = {}

        def hip():
            cent.copy_(init)
            out["hip"] = be.kmeans_fit(x, cent, ITERS)

        def composed():
            out["torch"] = lloyd_torch(x, init, ITERS)

        bodies = (("rsp_kmeans_fit (one call, 6 launches/iteration)", hip), ("torch composition (host loop, ~12 ops/iteration)", composed))
        for _, fn in bodies:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in bodies}
        for _ in range(args.repeats):
            for name, fn in bodies:
                times[name].append(timed(fn))
        torch.cuda.synchronize()
        info = cluster.read_info(out["hip"].info)
        obj = float(out["hip"].objective[info["iters_run"] - 1])
        same = float((out["hip"].assign.to(torch.int64) == out["torch"][1]).float().mean())
        lines.append(f"N {N} x D {D} -> {C} clusters (HIP fit: {info['iters_run']} iterations run, converged {info['converged']}, {info['empty']} "
                     f"empty, objective {obj:.6f}; torch after {ITERS}: objective {float(out['torch'][2]):.6f}; rows with the same final "
                     f"cluster {100 * same:.2f} %)")
        for name, _ in bodies:
            d, h = [v[0] for v in times[name]], [v[1] for v in times[name]]
            lines.append(f"  {name:<52}{statistics.median(d):10.3f} ({min(d):.3f} - {max(d):.3f}) | {statistics.median(h):8.3f}")
        del x, mu
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
